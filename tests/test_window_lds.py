"""CPU-only: the dynamic LDS of a launch of the three one-launch paths (single-chain windows, farm windows, chain runs) has
one home, window_lds_bytes / window_lds_fits in csrc/mgpu_internal.h.  The expressions the launch sites and capacity rules of
mgpu_windows.hip carried before are written out below as they stood -- the three narrow ones, chain_wide_lds, farm_wide_lds and
the two budget comparisons -- and compared with the shared functions, size and budget verdict, over: Coulomb tables of 48 to
65 536 bytes in steps of 48; nsplit 1..64; 0..32 pair entries (single-chain window) and 1..16 steps (chain run); the k role of
molecules of 1..5 sites (narrow) and 6..63 sites (wide) on test_chain_wide_lds.py's (ktot, n_rrows) grid, in the row, vector
and untiled matrix-unit forms.  A launch's size is the largest of three terms (pair role <- Coulomb table; k role; resolver <-
nsplit and the count): every k role is met at the ends and middle of the other axes; Coulomb table x nsplit x count is crossed in
full at three k roles; every 97th k role is crossed in full with nsplit x count and with the Coulomb table."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
#include <vector>
using namespace mgpu;
struct double2_ { double x, y; };
struct double4_ { double x, y, z, w; };
static const int kPairWaves = 8, kSiteChunk = 32, kFarmWideSites = 64, kMaxFusedSitesWide = 5;
static const size_t kFarmKFront = (size_t)kFarmWideSites * 3 * sizeof(double) + 2 * (size_t)kFarmWideSites * sizeof(double4_);
static const size_t kFarmWidePairBytes = (size_t)kPairWaves * ((kFarmWideSites * 3 + kSiteChunk * 4) * sizeof(double) + kSiteChunk * sizeof(int));

// ---- the engine as the former expressions saw it: its types' sizes as farm_type_form gave them (f.lds: a narrow type's row
// tables; kFarmKFront + the form's tables for a wide one), and recip_rows_lds_bytes(e, n1_max) of the narrow rows of a launch
struct Eng {
    size_t coul_bytes;
    int pair_nsplit, n_res, n1[2];
    size_t f_lds[2], rows_n1_max;
};
static size_t old_farm_resolver_scratch_bytes(int nsplit) { return (size_t)kPairWaves * (4 * nsplit + 4) * sizeof(double); }
static const size_t kOldFarmWideStaticMax = 16 * 1024, kOldFarmWideLdsMax = 160 * 1024 - kOldFarmWideStaticMax;
static size_t old_chain_wide_lds(const Eng *e) {
    size_t lds = chain_wide_pair_lds_bytes(e->coul_bytes, kPairWaves, kSiteChunk);
    for (int t = 0; t < e->n_res; ++t)
        lds = std::max(lds, e->n1[t] > kMaxFusedSitesWide ? chain_wide_k_lds_bytes(e->f_lds[t] - kFarmKFront) : e->f_lds[t]);
    return lds;
}
static size_t old_farm_wide_lds(const Eng *e) {
    size_t lds = ((e->coul_bytes + 15) & ~(size_t)15) + kFarmWidePairBytes;
    lds = std::max(lds, old_farm_resolver_scratch_bytes(e->pair_nsplit));
    for (int t = 0; t < e->n_res; ++t) lds = std::max(lds, e->f_lds[t]);
    return lds;
}
static size_t old_chain_lds(const Eng *e, bool wide, int n_ent) {
    const int nsplit = e->pair_nsplit;
    return std::max(wide ? old_chain_wide_lds(e) : std::max(e->coul_bytes, e->rows_n1_max), chain_resolver_lds_bytes(n_ent, nsplit));
}
static size_t old_farm_lds(const Eng *e, bool wide) {
    const int nsplit = e->pair_nsplit;
    return wide ? old_farm_wide_lds(e) : std::max(std::max(e->coul_bytes, e->rows_n1_max), old_farm_resolver_scratch_bytes(nsplit));
}
static size_t old_run_lds(const Eng *e, int k) {
    const int nsplit = e->pair_nsplit;
    return std::max(std::max(e->coul_bytes, e->rows_n1_max), chain_run_resolver_lds_bytes(k, nsplit));
}
static bool old_over(bool wide, size_t lds) { return lds > (wide ? kOldFarmWideLdsMax : kLdsDefaultMax); }
static bool old_over_default(size_t lds) { return lds > kLdsDefaultMax; }

static long long points, bad, n_path[3], n_side[2][2];       // [wide][over]
static void check(WindowPath path, bool wide, size_t was, size_t is) {
    ++points; ++n_path[path];
    const bool over = path == kPathRun ? old_over_default(was) : old_over(wide, was);
    ++n_side[wide][over];
    bad += was != is;
    bad += over == window_lds_fits(wide, is);
    bad += window_lds_budget(wide) != (wide ? kOldFarmWideLdsMax : kLdsDefaultMax);
}
// one engine at one count: every path, narrow and wide.  The table's entries as window_types_build fills them.
static void point(size_t coul, int nsplit, int count, size_t narrow_rows, int n1_wide, size_t wide_form) {
    Eng e{coul, nsplit, 2, {1, n1_wide}, {narrow_rows, kFarmKFront + wide_form}, narrow_rows};
    const size_t k_rows = window_k_lds_bytes(false, narrow_rows), k_max = std::max(k_rows, window_k_lds_bytes(true, wide_form));
    bad += farm_resolver_scratch_bytes(nsplit) != old_farm_resolver_scratch_bytes(nsplit);
    for (int wide = 0; wide < 2; ++wide) {
        const size_t k_bytes = wide ? k_max : k_rows;
        check(kPathFarm, wide, old_farm_lds(&e, wide), window_lds_bytes(kPathFarm, wide, coul, k_bytes, count, nsplit));
        if (count <= 32) check(kPathChain, wide, old_chain_lds(&e, wide, count), window_lds_bytes(kPathChain, wide, coul, k_bytes, count, nsplit));
    }
    if (count >= 1 && count <= 16) check(kPathRun, false, old_run_lds(&e, count), window_lds_bytes(kPathRun, false, coul, k_rows, count, nsplit));
}

struct KRole { size_t narrow_rows; int n1_wide; size_t wide_form; };

int main() {
    // ---- the k roles: test_chain_wide_lds.py's grid
    std::vector<KRole> roles;
    long long n_form[3] = {0, 0, 0}, n_narrow[6] = {0};
    for (int k0 = 2; k0 <= 24; k0 += 2)
        for (int k1 = 2; k1 <= 24; k1 += 3)
            for (int k2 = 2; k2 <= 24; k2 += 5) {
                const int ktot = k0 + k1 + k2 + 3;
                const int full = (k0 + 1) * (2 * k1 + 1) - k1 - 1;
                for (int n_rrows : {full, (full + 1) / 2})
                    for (int n1 = 6; n1 < kFarmWideSites; ++n1) {
                        const int n1_narrow = 1 + (n1 + k0 + k1) % 5;
                        const size_t narrow_rows = recip_rows_lds_bytes(ktot, n_rrows, n1_narrow);
                        ++n_narrow[n1_narrow];
                        roles.push_back(KRole{narrow_rows, n1, recip_rows_lds_bytes(ktot, n_rrows, n1)});
                        ++n_form[0];
                        const int rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                        if (rpt) { roles.push_back(KRole{narrow_rows, n1, recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false)}); ++n_form[1]; }
                        const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1);
                        if (mt >= ((2 * n1 + 3) & ~3)) { roles.push_back(KRole{narrow_rows, n1, recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true)}); ++n_form[2]; }
                    }
            }
    const size_t coul_ends[3] = {48, 48 * 683, 48 * 1365};
    const int nsplit_ends[3] = {1, 7, 64}, count_ends[3] = {0, 9, 32};
    const KRole role_ends[3] = {roles.front(), roles[roles.size() / 2], KRole{0, 6, 0}};
    // every k role at the ends and middle of the other axes
    for (const KRole &r : roles)
        for (size_t coul : coul_ends)
            for (int nsplit : nsplit_ends)
                for (int count : count_ends) point(coul, nsplit, count, r.narrow_rows, r.n1_wide, r.wide_form);
    // pair role x resolver, in full
    for (size_t coul = 48; coul <= kLdsDefaultMax; coul += 48)
        for (int nsplit = 1; nsplit <= 64; ++nsplit)
            for (int count = 0; count <= 32; ++count)
                for (const KRole &r : role_ends) point(coul, nsplit, count, r.narrow_rows, r.n1_wide, r.wide_form);
    // every 97th k role (a stride prime to the grid's inner loops: every site count, form and kmax turns up) x resolver and
    // x pair role, in full
    for (size_t i = 0; i < roles.size(); i += 97) {
        const KRole &r = roles[i];
        for (int nsplit = 1; nsplit <= 64; ++nsplit)
            for (int count = 0; count <= 32; ++count)
                for (size_t coul : coul_ends) point(coul, nsplit, count, r.narrow_rows, r.n1_wide, r.wide_form);
        for (size_t coul = 48; coul <= kLdsDefaultMax; coul += 48)
            for (int j = 0; j < 3; ++j) point(coul, nsplit_ends[j], count_ends[j], r.narrow_rows, r.n1_wide, r.wide_form);
    }
    long long narrow_sizes = 0;
    for (int n1 = 1; n1 <= 5; ++n1) narrow_sizes += n_narrow[n1] > 0;
    std::printf("points %lld bad %lld chain %lld farm %lld run %lld rows %lld vector %lld mfma %lld narrow_site_counts %lld "
                "narrow_within %lld narrow_over %lld wide_within %lld wide_over %lld\n",
                points, bad, n_path[kPathChain], n_path[kPathFarm], n_path[kPathRun], n_form[0], n_form[1], n_form[2], narrow_sizes,
                n_side[0][0], n_side[0][1], n_side[1][0], n_side[1][1]);
    return bad != 0;
}
"""


def test_window_lds_plan_equals_the_launch_sites_former_expressions(tmp_path):
    src = tmp_path / "window_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "window_lds"
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert out.returncode == 0 and fields[:1] == ["points"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert counts["points"] > 0 and counts["bad"] == 0, out.stdout
    # every path, every form and each side of each budget was met, so that none of the comparisons above was vacuous
    for key in ("chain", "farm", "run", "rows", "vector", "mfma", "narrow_within", "narrow_over", "wide_within", "wide_over"):
        assert counts[key] > 0, (key, out.stdout)
    assert counts["narrow_site_counts"] == 5, out.stdout
