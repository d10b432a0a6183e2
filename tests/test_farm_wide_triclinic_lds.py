"""CPU-only: the dynamic LDS of the image-search WIDE farm launch (farm_window_kernel<false, false, true, RSV, true>) is
window_lds_bytes(kPathFarm, true, ...) of csrc/mgpu_internal.h with WindowTypes::k_lds_max_tri -- the roles stage what the
orthorhombic WIDE roles stage (candidate row and slabs behind the Coulomb table, the k role of the type's own form behind
kFarmKFront, the resolving waves' scratch), so the formula has no new case.  Over tests/test_window_lds.py's grid -- the k role of
molecules of 1..5 sites (narrow) and 6..63 sites (wide) on test_chain_wide_lds.py's (ktot, n_rrows) grid in the row, vector and
untiled matrix-unit forms; Coulomb tables of 48 to 65 536 bytes; nsplit 1..64; 0..32 chains -- k_lds_max_tri as window_types_build
forms it for a triclinic box (the max over the narrow type and the type of 6..63 sites, which goes to take_tri) is k_lds_max as it
forms it for the same types in an orthorhombic box, and the launch's size and budget verdict are the orthorhombic WIDE farm's,
written out from the kernel's pointer arithmetic.  The launch site reads the farm's own switch and names the two new instances in
its opt-in list; the kernel holds the assertion that the image search has no flat form and no fast fold."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
#include <vector>
using namespace mgpu;
static const size_t D = sizeof(double);
static const int kWaves = 8, kChunk = 32, kSites = 64;     // kPairWaves, kSiteChunk, kFarmWideSites
static const size_t kFront = (size_t)kSites * 3 * D + 2 * (size_t)kSites * 4 * D;
// the orthorhombic WIDE farm launch, from the kernel's pointer arithmetic: pair role | k role | resolving waves
static size_t ortho_wide_farm(size_t coul, size_t narrow_rows, size_t wide_form, int nsplit) {
    size_t lds = ((coul + 15) & ~(size_t)15) + (size_t)kWaves * ((kSites * 3 + kChunk * 4) * D + kChunk * sizeof(int));
    lds = std::max(lds, (size_t)kWaves * (4 * nsplit + 4) * D);
    lds = std::max(lds, narrow_rows);
    return std::max(lds, kFront + wide_form);
}
// window_types_build's maxima for a box with a narrow type and a type of 6..63 sites: orthorhombic (both go to take), triclinic
// (the narrow one to take, the other to take_tri)
struct Maxima { size_t k_lds_max, k_lds_max_tri; };
static Maxima types_build(bool triclinic, size_t narrow_rows, size_t wide_form) {
    Maxima m{0, 0};
    const size_t k_lds[2] = {window_k_lds_bytes(false, narrow_rows), window_k_lds_bytes(true, wide_form)};
    for (int t = 0; t < 2; ++t) {
        m.k_lds_max_tri = std::max(m.k_lds_max_tri, k_lds[t]);
        if (t == 1 && triclinic) continue;
        m.k_lds_max = std::max(m.k_lds_max, k_lds[t]);
    }
    return m;
}
static long long points, bad, within, over;
static void point(size_t coul, int nsplit, int count, size_t narrow_rows, size_t wide_form) {
    const Maxima tri = types_build(true, narrow_rows, wide_form), ortho = types_build(false, narrow_rows, wide_form);
    bad += tri.k_lds_max_tri != ortho.k_lds_max || ortho.k_lds_max_tri != ortho.k_lds_max;
    bad += tri.k_lds_max != window_k_lds_bytes(false, narrow_rows);          // (without the switch: the narrow type alone)
    const size_t is = window_lds_bytes(kPathFarm, true, coul, tri.k_lds_max_tri, count, nsplit);
    const size_t was = window_lds_bytes(kPathFarm, true, coul, ortho.k_lds_max, count, nsplit);
    bad += is != was || is != ortho_wide_farm(coul, narrow_rows, wide_form, nsplit);
    const bool fits = is <= (size_t)160 * 1024 - 16 * 1024;
    bad += fits != window_lds_fits(true, is) || window_lds_budget(true) != kFarmWideLdsMax;
    ++points; ++(fits ? within : over);
}
struct KRole { size_t narrow_rows, wide_form; };

int main() {
    std::vector<KRole> roles;
    long long n_form[3] = {0, 0, 0};
    for (int k0 = 2; k0 <= 24; k0 += 2)
        for (int k1 = 2; k1 <= 24; k1 += 3)
            for (int k2 = 2; k2 <= 24; k2 += 5) {
                const int ktot = k0 + k1 + k2 + 3;
                const int full = (k0 + 1) * (2 * k1 + 1) - k1 - 1;
                for (int n_rrows : {full, (full + 1) / 2})
                    for (int n1 = 6; n1 < kSites; ++n1) {
                        const size_t narrow_rows = recip_rows_lds_bytes(ktot, n_rrows, 1 + (n1 + k0 + k1) % 5);
                        roles.push_back(KRole{narrow_rows, recip_rows_lds_bytes(ktot, n_rrows, n1)});
                        ++n_form[0];
                        const int rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                        if (rpt) { roles.push_back(KRole{narrow_rows, recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false)}); ++n_form[1]; }
                        const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1);
                        if (mt >= ((2 * n1 + 3) & ~3)) { roles.push_back(KRole{narrow_rows, recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true)}); ++n_form[2]; }
                    }
            }
    const size_t coul_ends[3] = {48, 48 * 683, 48 * 1365};
    const int nsplit_ends[3] = {1, 7, 64}, count_ends[3] = {0, 9, 32};
    // every k role at the ends and middle of the other axes
    for (const KRole &r : roles)
        for (size_t coul : coul_ends)
            for (int nsplit : nsplit_ends)
                for (int count : count_ends) point(coul, nsplit, count, r.narrow_rows, r.wide_form);
    // every 97th k role x resolver and x pair role, in full
    for (size_t i = 0; i < roles.size(); i += 97) {
        const KRole &r = roles[i];
        for (int nsplit = 1; nsplit <= 64; ++nsplit)
            for (int count = 0; count <= 32; ++count)
                for (size_t coul : coul_ends) point(coul, nsplit, count, r.narrow_rows, r.wide_form);
        for (size_t coul = 48; coul <= kLdsDefaultMax; coul += 48)
            for (int j = 0; j < 3; ++j) point(coul, nsplit_ends[j], count_ends[j], r.narrow_rows, r.wide_form);
    }
    std::printf("points %lld bad %lld rows %lld vector %lld mfma %lld within %lld over %lld\n", points, bad, n_form[0], n_form[1],
                n_form[2], within, over);
    return bad != 0;
}
"""


def test_the_tilted_wide_farm_launch_is_the_orthorhombic_wide_farms_size(tmp_path):
    src = tmp_path / "farm_wide_triclinic_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "farm_wide_triclinic_lds"
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert out.returncode == 0 and fields[:1] == ["points"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert counts["points"] > 0 and counts["bad"] == 0, out.stdout
    for key in ("rows", "vector", "mfma", "within", "over"):            # every form and each side of the budget was met
        assert counts[key] > 0, (key, out.stdout)


def test_the_launch_site_reads_the_farms_switch_and_names_the_instances():
    csrc = os.path.join(ROOT, "maniac_mc_amd", "csrc")
    hdr = " ".join(open(os.path.join(csrc, "mgpu_kernels_windows.h")).read().split())
    assert "template <bool RSV, bool TRI = false> __device__ __forceinline__ void farm_wide_pair_unit(" in hdr
    assert "template <bool RSV, bool TRI = false> __device__ __forceinline__ void farm_wide_k_role(" in hdr
    assert "farm_wide_k_role<RSV, TRI>(" in hdr and "farm_wide_pair_unit<RSV, TRI>(" in hdr
    assert "trial_frame<RSV>(" not in hdr                                # every place that rebuilds a row takes the kernel's TRI
    kernel = hdr[hdr.index("void farm_window_kernel("):hdr.index("// Chain runs:")]
    assert 'static_assert(!TRI || (!FLAT && !FASTW), "the image search has no flat form and no fast fold, with WIDE or without");' in kernel
    assert "#define MGPU_FARM_WIDE_MINWAVES 2 " in hdr                    # (not moved)
    win = " ".join(open(os.path.join(csrc, "mgpu_windows.hip")).read().split())
    tri = win[win.index("static bool window_tri_wide("):win.index("static bool window_takes_wide(")]
    assert "path != kPathFarm ? e->wide_tri : e->farm_wide_tri" in tri
    lds = win[win.index("static size_t window_lds("):win.index("static void wide_args(")]
    assert "window_tri_wide(e, path) ? e->win.k_lds_max_tri : e->win.k_lds_max" in lds
    submit = win[win.index("int mgpu_farm_window_submit("):win.index("int mgpu_farm_window_wait(")]
    assert "wide = wide || window_takes_wide(e, kPathFarm, t[c]);" in submit
    assert "f(farm_window_kernel<false, false, decltype(WIDE)::value, decltype(RSV)::value, true>);" in submit
    opt = submit[submit.index("lds_opt_in(e->device, kLdsFarmWide"):submit.index("fw.seq += 1;")]
    assert "tri_family(f, std::true_type{}, RSV)" in opt
    assert "tri_family(launch, flags...); }, wide, e->rsv_any);" in submit
    eng = open(os.path.join(csrc, "mgpu_engine.h")).read()
    assert "bool farm_wide_tri = false;" in eng                          # off at creation
