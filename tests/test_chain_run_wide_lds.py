"""CPU-only: the dynamic LDS of a WIDE chain-run launch (chain_run_kernel<..., WIDE>) is window_lds_bytes(kPathRun, true, ...)
of csrc/mgpu_internal.h -- the largest of its three roles' needs.  The byte each role indexes last is written out below from
the kernel's own pointer arithmetic (wide_pair_lds for the pair role's rows and slabs behind the Coulomb table; wide_k_sweep's
row, intra tiles and tables; the resolver's staging of 4 nsplit doubles per step) and compared over a grid of Coulomb-table
sizes, forms, k = 1..16 and nsplit; the launch of the test boxes (6, 8, 24, 40 sites at L = 26, the 3 + 24 mixture at L = 36:
their tables and k-vector counts are written out here from the engine's setup rule) is within kFarmWideLdsMax; and the narrow
launch's size is what it was: max(Coulomb table, row-form tables, resolver)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
using namespace mgpu;
static const size_t D = sizeof(double), D2 = 2 * sizeof(double), D4 = 4 * sizeof(double), I4 = 4 * sizeof(int);
static const int kWaves = 8, kChunk = 32, kSites = 64;     // kPairWaves, kSiteChunk, kFarmWideSites
static size_t k_front_end() { return kSites * 3 * D + kSites * D4 + kSites * D4; }
static size_t rows_end(int ktot, int n_rows, int n1) { return (size_t)2 * n1 * ktot * D2 + (size_t)n1 * D + (size_t)n_rows * 2 * n1 * D2; }
static size_t wide_end(int ktot, int n_rows, size_t nss, int rpt, bool mfma) {
    return nss * ktot * D2 + (size_t)rpt * nss * D2 + nss * D + (mfma ? (size_t)n_rows * I4 : 0);
}
// wide_pair_lds: slab = s_dyn + wide_at; cand = slab + wave kSites 3; w_site = slab + kWaves kSites 3 + wave kChunk 4;
// w_sty = (int *)(slab + kWaves (kSites 3 + kChunk 4)) + wave kChunk: the last wave's last entry
static size_t pair_end(size_t coul_bytes) {
    const size_t at = (coul_bytes + 15) & ~(size_t)15;
    return at + (size_t)kWaves * (kSites * 3 + kChunk * 4) * D + (size_t)kWaves * kChunk * sizeof(int);
}
// the resolver: st[i], i < per cnt, per = 4 nsplit doubles
static size_t resolver_end(int k, int nsplit) { return (size_t)4 * nsplit * k * D; }
static size_t max3(size_t a, size_t b, size_t c) { return std::max(a, std::max(b, c)); }

int main() {
    long long points = 0, bad = 0, rows = 0, vec = 0, mfma = 0, over = 0;
    for (size_t coul = 48; coul <= kLdsDefaultMax; coul += 48 * 37)
        for (int nsplit : {1, 2, 3, 4, 8, 16, 32, 64})
            for (int k = 1; k <= std::min(16, chain_window_steps_by_lds(nsplit)); ++k) {
                // the narrow launch: unchanged
                for (size_t k_rows : {(size_t)0, (size_t)4096, (size_t)40 * 1024}) {
                    bad += window_lds_bytes(kPathRun, false, coul, k_rows, k, nsplit) != max3(coul, k_rows, resolver_end(k, nsplit));
                    bad += window_lds_bytes(kPathRun, false, coul, k_rows, k, nsplit) > kLdsDefaultMax;
                }
                for (int ktot : {9, 21, 33, 45})
                    for (int n_rrows : {40, 220, 600})
                        for (int n1 : {6, 8, 12, 24, 40, 63}) {
                            // every form recip_plan may give the type: rows while they fit, else untiled matrix-unit and / or vector
                            size_t form[2] = {0, 0}, want[2] = {0, 0};
                            if (recip_rows_lds_bytes(ktot, n_rrows, n1) <= kRecipRowsLdsMax) {
                                ++rows;
                                form[0] = recip_rows_lds_bytes(ktot, n_rrows, n1); want[0] = rows_end(ktot, n_rrows, n1);
                            } else {
                                const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1), rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                                if (mt >= ((2 * n1 + 3) & ~3)) {
                                    ++mfma;
                                    form[0] = recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true); want[0] = wide_end(ktot, n_rrows, mt, 0, true);
                                }
                                if (rpt) {
                                    ++vec;
                                    form[1] = recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false); want[1] = wide_end(ktot, n_rrows, 2 * n1, rpt, false);
                                }
                            }
                            for (int f = 0; f < 2; ++f) {
                                if (!form[f]) continue;
                                ++points;
                                const size_t k_bytes = window_k_lds_bytes(true, form[f]);
                                bad += k_bytes != k_front_end() + want[f];
                                const size_t lds = window_lds_bytes(kPathRun, true, coul, k_bytes, k, nsplit);
                                bad += lds != max3(pair_end(coul), k_front_end() + want[f], resolver_end(k, nsplit));
                                over += !window_lds_fits(true, lds);
                                bad += window_lds_fits(true, lds) != (lds <= kFarmWideLdsMax);
                            }
                        }
            }
    // the test boxes: rc = 10 A, tolerance 1e-5 -> Coulomb tables of at most 48 KiB and kmax <= 10 per axis at L <= 36 A (ktot <= 33,
    // at most (kmax + 1)(2 kmax + 1) - kmax - 1 = 220 rows); every form the plan can give 6 .. 40 sites there
    for (int n1 : {6, 8, 12, 24, 40})
        for (int ktot : {21, 27, 33})
            for (int n_rrows : {112, 220}) {
                size_t form = recip_rows_lds_bytes(ktot, n_rrows, n1);
                if (form > kRecipRowsLdsMax) {
                    const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1), rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                    const size_t fm = mt >= ((2 * n1 + 3) & ~3) ? recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true) : 0;
                    const size_t fv = rpt ? recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false) : 0;
                    form = std::max(fm, fv);
                    bad += form == 0;
                }
                for (int nsplit : {1, 4, 16})
                    bad += !window_lds_fits(true, window_lds_bytes(kPathRun, true, 48 * 1024, window_k_lds_bytes(true, form), 16, nsplit));
            }
    bad += kFarmWideLdsMax != 160 * 1024 - 16 * 1024;
    std::printf("points %lld bad %lld rows %lld vector %lld mfma %lld over %lld\n", points, bad, rows, vec, mfma, over);
    return bad != 0;
}
"""


def test_wide_chain_run_lds_is_the_largest_of_its_roles(tmp_path):
    src = tmp_path / "chain_run_wide_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "chain_run_wide_lds"
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert out.returncode == 0 and fields[:1] == ["points"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert counts["points"] > 0 and counts["bad"] == 0, out.stdout
    assert counts["rows"] > 0 and counts["vector"] > 0 and counts["mfma"] > 0, out.stdout


def test_the_kernel_header_reads_what_the_launch_fills():
    """ChainRunArgs carries ChainArgs's five WIDE fields, the 4 KB assertion stands, and the launch site fills them with wide_args
    and opts in through a family of its own."""
    csrc = os.path.join(ROOT, "maniac_mc_amd", "csrc")
    hdr = open(os.path.join(csrc, "mgpu_kernels_windows.h")).read()
    body = hdr[hdr.index("struct ChainRunArgs {"):hdr.index("a chain-run launch must fit the kernel-argument segment")]
    for field in ("const int *row_first;", "int wide_at;", "signed char kform[kMaxRes];", "int wide_rpt[kMaxRes];", "int wide_nss[kMaxRes];"):
        assert field in body, field
    assert "sizeof(BoxDev) + sizeof(ChainRunArgs) + 160 <= 4096" in body
    assert "static_assert(!(WIDE && TRI)" in hdr
    win = open(os.path.join(csrc, "mgpu_windows.hip")).read()
    assert "kLdsRunWide" in win and "wide_args(e, &g.row_first, &g.wide_at, g.kform, g.wide_rpt, g.wide_nss)" in win
    assert "window_lds(e, kPathRun, wide, k_rows, rn.k)" in win
