"""CPU-only: the dynamic LDS of the image-search WIDE launches (chain_window_kernel<false, false, true, true>,
chain_run_kernel<false, false, true, GC, true>) is window_lds_bytes(kPathChain | kPathRun, true, ...) of csrc/mgpu_internal.h -- the
roles stage what the orthorhombic WIDE roles stage, so the formula has no new case; what is new is the boxes.  A stand-alone host
program over mgpu_internal.h and the engine's own setup rule (mgpu_host_setup.cpp: box_prepare, ewald_setup, ewald_kvectors,
build_coulomb_table with the triclinic table's range (|a| + |b| + |c|)^2) works out, for the tilted test boxes -- 6, 24 and 40
sites at L = 26 A and the 3 + 24 mixture at L = 36 A under the mild tilt, the sheared 18 x 21 x 24 A cell, and the mixture in 1.5 times that cell -- the Coulomb
table, the k-vector rows and the k role of every form the plan can give the type (tests/test_chain_run_wide_lds.py's byte counts,
written out from the kernel's pointer arithmetic), and checks that every launch is within kFarmWideLdsMax for both paths and that
the table stays within 64 KiB.  The header still holds the narrowed assertion, and the launch sites name the new instances in
their opt-in lists."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cmath>
#include <cstdio>
namespace mgpu { int set_error(int code, const std::string &msg) { std::fprintf(stderr, "%s\n", msg.c_str()); return code; } }
using namespace mgpu;
static const size_t D = sizeof(double), D2 = 2 * sizeof(double), D4 = 4 * sizeof(double), I4 = 4 * sizeof(int);
static const int kWaves = 8, kChunk = 32, kSites = 64;     // kPairWaves, kSiteChunk, kFarmWideSites
static size_t k_front_end() { return kSites * 3 * D + kSites * D4 + kSites * D4; }
static size_t rows_end(int ktot, int n_rows, int n1) { return (size_t)2 * n1 * ktot * D2 + (size_t)n1 * D + (size_t)n_rows * 2 * n1 * D2; }
static size_t wide_end(int ktot, int n_rows, size_t nss, int rpt, bool mfma) {
    return nss * ktot * D2 + (size_t)rpt * nss * D2 + nss * D + (mfma ? (size_t)n_rows * I4 : 0);
}
static size_t pair_end(size_t coul_bytes) {
    const size_t at = (coul_bytes + 15) & ~(size_t)15;
    return at + (size_t)kWaves * (kSites * 3 + kChunk * 4) * D + (size_t)kWaves * kChunk * sizeof(int);
}
static size_t max3(size_t a, size_t b, size_t c) { return std::max(a, std::max(b, c)); }

struct Box { const char *name; double m[9]; int n1[2]; };

int main() {
    // rows a = (lx, 0, 0), b = (xy, ly, 0), c = (xz, yz, lz)
    const Box boxes[] = {
        {"mild 6", {26, 0, 0, 1.5, 26, 0, -0.8, 0.6, 26}, {6, 0}},
        {"mild 24", {26, 0, 0, 1.5, 26, 0, -0.8, 0.6, 26}, {24, 0}},
        {"mild 40", {26, 0, 0, 1.5, 26, 0, -0.8, 0.6, 26}, {40, 0}},
        {"mild 3 + 24", {36, 0, 0, 1.5, 36, 0, -0.8, 0.6, 36}, {3, 24}},
        {"sheared 6", {18, 0, 0, 8.9, 21, 0, -11.9, 10.4, 24}, {6, 0}},
        {"sheared 24", {18, 0, 0, 8.9, 21, 0, -11.9, 10.4, 24}, {24, 0}},
        {"sheared 40", {18, 0, 0, 8.9, 21, 0, -11.9, 10.4, 24}, {40, 0}},
        {"sheared 3 + 24", {27, 0, 0, 13.35, 31.5, 0, -17.85, 15.6, 36}, {3, 24}},
    };
    long long bad = 0, launches = 0, rows_f = 0, vec_f = 0, mfma_f = 0;
    for (const Box &b : boxes) {
        int box_type = 0, kmax[3] = {0, 0, 0}, nk = 0;
        double volume = 0, rcp[9], metrics[9], rc = 10.0, tol = 1e-5, alpha = 0, screening = 0, fprec = 0;
        if (box_prepare(b.m, &box_type, &volume, rcp, metrics)) return 2;
        if (ewald_setup(metrics, &rc, &tol, &alpha, &screening, &fprec, kmax, &nk)) return 2;
        std::vector<int> kx(nk), ky(nk), kz(nk);
        std::vector<double> k2(nk), ff(nk), w(nk);
        if (ewald_kvectors(rcp, alpha, kmax, nk, kx.data(), ky.data(), kz.data(), k2.data(), ff.data(), w.data())) return 2;
        int n_rrows = 0;
        for (int i = 0; i < nk; ++i) n_rrows += i == 0 || kx[i] != kx[i - 1] || ky[i] != ky[i - 1];
        const double sum_len = metrics[0] + metrics[1] + metrics[2];
        std::vector<CoulRow> rows;
        int idx_base = 0;
        if (build_coulomb_table(alpha, std::max(sum_len * sum_len, 1.0), rows, &idx_base)) return 2;
        const size_t coul = rows.size() * sizeof(CoulRow);
        const int ktot = recip_ktot(kmax);
        bad += coul > kLdsDefaultMax;                      // (a larger table keeps capacity 0)
        // the largest k role over the types a row may carry, in the matrix-unit plan [0] and under MGPU_RECIP_NO_MFMA [1]
        size_t k_max[2] = {0, 0};
        for (int n1 : b.n1) {
            if (!n1) continue;
            const bool wide = n1 > 5;
            size_t form[2] = {0, 0}, want[2] = {0, 0};
            if (recip_rows_lds_bytes(ktot, n_rrows, n1) <= kRecipRowsLdsMax) {
                ++rows_f;
                form[0] = form[1] = recip_rows_lds_bytes(ktot, n_rrows, n1);
                want[0] = want[1] = rows_end(ktot, n_rrows, n1);
            } else {
                const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1), rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                bad += !wide;                              // (the narrow type of the mixture takes the row form)
                if (mt >= ((2 * n1 + 3) & ~3)) {
                    ++mfma_f;
                    form[0] = recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true); want[0] = wide_end(ktot, n_rrows, mt, 0, true);
                }
                if (rpt) {
                    ++vec_f;
                    form[1] = recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false); want[1] = wide_end(ktot, n_rrows, 2 * n1, rpt, false);
                }
                if (!form[0]) { form[0] = form[1]; want[0] = want[1]; }
                bad += !form[0] || !form[1];               // (the test boxes' types are admitted in both plans)
            }
            for (int f = 0; f < 2; ++f) {
                bad += window_k_lds_bytes(wide, form[f]) != (wide ? k_front_end() : 0) + want[f];
                k_max[f] = std::max(k_max[f], window_k_lds_bytes(wide, form[f]));
            }
        }
        for (int f = 0; f < 2; ++f)
            for (int nsplit : {1, 2, 4, 8, 16}) {
                const int cap = std::min(16, chain_window_steps_by_lds(nsplit));
                // a single-chain window of `cap` steps carries up to two pair entries per step; a run launch up to 16 steps
                const size_t chain = window_lds_bytes(kPathChain, true, coul, k_max[f], 2 * cap, nsplit);
                const size_t run = window_lds_bytes(kPathRun, true, coul, k_max[f], cap, nsplit);
                bad += chain != max3(pair_end(coul), k_max[f], (size_t)2 * cap * nsplit * D2);
                bad += run != max3(pair_end(coul), k_max[f], (size_t)4 * nsplit * cap * D);
                bad += !window_lds_fits(true, chain) || !window_lds_fits(true, run);
                bad += chain > kFarmWideLdsMax || run > kFarmWideLdsMax;
                launches += 2;
            }
        std::printf("# %s: kmax %d %d %d, rows %d, Coulomb table %zu bytes, k role %zu / %zu bytes\n", b.name, kmax[0], kmax[1], kmax[2],
                    n_rrows, coul, k_max[0], k_max[1]);
    }
    bad += kFarmWideLdsMax != 160 * 1024 - 16 * 1024;
    std::printf("launches %lld bad %lld rows %lld vector %lld mfma %lld\n", launches, bad, rows_f, vec_f, mfma_f);
    return bad != 0;
}
"""


def test_the_tilted_boxes_launches_fit_the_wide_budget(tmp_path):
    src = tmp_path / "wide_triclinic_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "wide_triclinic_lds"
    csrc = os.path.join(ROOT, "maniac_mc_amd", "csrc")
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-fopenmp", "-I", csrc, str(src), os.path.join(csrc, "mgpu_host_setup.cpp"),
                                 "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    last = out.stdout.strip().split("\n")[-1].split()
    assert out.returncode == 0 and last[:1] == ["launches"], out.stdout + out.stderr
    counts = dict(zip(last[0::2], map(int, last[1::2])))
    assert counts["launches"] == 8 * 2 * 5 * 2 and counts["bad"] == 0, out.stdout
    assert counts["rows"] > 0 and counts["vector"] > 0 and counts["mfma"] > 0, out.stdout


def test_the_header_holds_the_narrowed_assertion_and_the_launch_sites_name_the_instances():
    csrc = os.path.join(ROOT, "maniac_mc_amd", "csrc")
    hdr = open(os.path.join(csrc, "mgpu_kernels_windows.h")).read()
    assert "static_assert(!(WIDE && TRI) || (!FLAT && !FASTW)," in hdr
    assert "template <bool TRI>\n__device__ __forceinline__ void chain_wide_pair_unit(" in hdr
    assert hdr.count("pair_sweep_item<0, false, TRI, false, false, true>") == 2       # the window's and the run's WIDE pair unit
    assert "trial_frame<false>(" not in hdr                                          # the run rebuilds every row with its TRI
    win = open(os.path.join(csrc, "mgpu_windows.hip")).read()
    flat = " ".join(win.split())
    # the opt-in lists of the two single-chain WIDE families name the image-search instances, and the launch sites pick them
    chain_opt = flat[flat.index("lds_opt_in(e->device, kLdsChainWide"):flat.index("ch.seq += 1;")]
    assert "tri_wide_family(f)" in chain_opt
    run_opt = flat[flat.index("lds_opt_in(e->device, kLdsRunWide"):flat.index("ChainRunArgs g{};")]
    assert "tri_wide_family(f, flags...)" in run_opt
    assert "f(chain_window_kernel<false, false, true, true>)" in flat
    assert "f(chain_run_kernel<false, false, true, decltype(GC)::value, true>)" in flat
    assert "if (e->bx.triclinic && wide) tri_wide_family(launch);" in flat
    assert "if (e->bx.triclinic && wide) with_bools([&](auto... flags) { tri_wide_family(launch, flags...); }, rn.gc);" in flat
    # the farm's admission does not read the switch
    farm = flat[flat.index("static bool window_tri_wide("):flat.index("static bool window_takes_wide(")]
    assert "path != kPathFarm" in farm
    assert not re.search(r"farm_window_kernel<[^>]*>[^;]*tri_wide", flat)
