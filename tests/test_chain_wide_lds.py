"""CPU-only: the dynamic-LDS sizes of the WIDE single-chain windows (chain_window_kernel<..., WIDE>) have one home
(csrc/mgpu_internal.h); a size that disagrees with the kernel's layout is an out-of-bounds LDS access.  The byte each role
indexes last is written out below from the kernel's own pointer arithmetic (chain_wide_k_role, chain_wide_pair_unit, the
resolver's staging; recip_rows_tables / recip_wide_sweep for the tables) and compared with the shared functions over
everything such a window admits: 6..63 sites, the row form and both untiled wide forms, nsplit 1..64, Coulomb tables up to
64 KiB.  Also: the whole-run fixtures of these molecules list exactly the files that are there."""
import json
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

// k role: cand = s_dyn; intra_a = s_dyn + kSites 3 doubles; intra_b = intra_a + kSites (double4); tabs behind them
static size_t k_front_end() { return kSites * 3 * D + kSites * D4 + kSites * D4; }
// row form (recip_lds_view): tab [2 n1][ktot] double2 | charges [n1] | xy [rows][2 n1] double2
static size_t rows_end(int ktot, int n_rows, int n1) { return (size_t)2 * n1 * ktot * D2 + (size_t)n1 * D + (size_t)n_rows * 2 * n1 * D2; }
// recip_wide_sweep: tab = s_tab [nss_max][ktot]; xyt = tab + nss_max ktot, [rpt][nss_max]; sq = (double *)(xyt + rpt nss_max), [nss_max];
// rowmeta = (int4 *)(sq + nss_max), [n_rows] (matrix-unit form)
static size_t wide_end(int ktot, int n_rows, size_t nss, int rpt, bool mfma) {
    return nss * ktot * D2 + (size_t)rpt * nss * D2 + nss * D + (mfma ? (size_t)n_rows * I4 : 0);
}
// pair role: slab = s_dyn + wide_at; cand = slab + wave kSites 3; w_site = slab + kWaves kSites 3 + wave kChunk 4;
// w_sty = (int *)(slab + kWaves (kSites 3 + kChunk 4)) + wave kChunk: the last wave's last entry
static size_t pair_end(size_t coul_bytes) {
    const size_t at = (coul_bytes + 15) & ~(size_t)15;
    return at + (size_t)kWaves * (kSites * 3 + kChunk * 4) * D + ((size_t)(kWaves - 1) * kChunk + kChunk) * sizeof(int);
}

int main() {
    long long points = 0, bad = 0, rows = 0, vec = 0, mfma = 0, refused = 0;
    bad += wide_k_front_bytes() != k_front_end();
    bad += kWideRowSites != kSites;
    for (size_t coul = 48; coul <= kLdsDefaultMax; coul += 48) {          // whole table rows
        bad += chain_wide_pair_lds_bytes(coul, kWaves, kChunk) != pair_end(coul);
        bad += chain_wide_pair_at(coul) % 16 != 0 || chain_wide_pair_at(coul) < coul;
    }
    for (int nsplit = 1; nsplit <= 64; ++nsplit) {
        const int cap = std::min(16, chain_window_steps_by_lds(nsplit));
        for (int n_ent = 0; n_ent <= 2 * cap; ++n_ent) {
            // st[i], i < 2 np doubles, np = n_ent nsplit
            bad += chain_resolver_lds_bytes(n_ent, nsplit) != (size_t)2 * n_ent * nsplit * D;
            bad += chain_resolver_lds_bytes(n_ent, nsplit) > kLdsDefaultMax;
        }
    }
    for (int k0 = 2; k0 <= 24; k0 += 2)
        for (int k1 = 2; k1 <= 24; k1 += 3)
            for (int k2 = 2; k2 <= 24; k2 += 5) {
                const int ktot = k0 + k1 + k2 + 3;
                const int full = (k0 + 1) * (2 * k1 + 1) - k1 - 1;
                for (int n_rrows : {full, (full + 1) / 2})
                    for (int n1 = 6; n1 < kSites; ++n1) {
                        ++points;
                        // the form recip_plan gives the type: rows while they fit, else untiled matrix-unit, else vector
                        if (recip_rows_lds_bytes(ktot, n_rrows, n1) <= kRecipRowsLdsMax) {
                            ++rows;
                            bad += chain_wide_k_lds_bytes(recip_rows_lds_bytes(ktot, n_rrows, n1)) != k_front_end() + rows_end(ktot, n_rrows, n1);
                            continue;
                        }
                        const int mt = recip_wide_mfma_tile(ktot, n_rrows, n1);
                        if (mt >= ((2 * n1 + 3) & ~3)) {
                            ++mfma;
                            bad += chain_wide_k_lds_bytes(recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true)) != k_front_end() + wide_end(ktot, n_rrows, mt, 0, true);
                            bad += mt < 2 * n1;            // every site-state has its table
                        }
                        const int rpt = recip_wide_rows_per_tile(ktot, n_rrows, n1);
                        if (rpt) {
                            ++vec;
                            bad += chain_wide_k_lds_bytes(recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false)) !=
                                   k_front_end() + wide_end(ktot, n_rrows, 2 * n1, rpt, false);
                        }
                        if (!rpt && mt < ((2 * n1 + 3) & ~3)) ++refused;
                    }
            }
    std::printf("points %lld bad %lld rows %lld vector %lld mfma %lld refused %lld\n", points, bad, rows, vec, mfma, refused);
    return bad != 0;
}
"""


def test_wide_chain_window_lds_sizes_are_the_kernels_layout(tmp_path):
    src = tmp_path / "chain_wide_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "chain_wide_lds"
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert out.returncode == 0 and fields[:1] == ["points"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert counts["points"] > 0 and counts["bad"] == 0, out.stdout
    # every admitted form was met, so that none of the comparisons above was vacuous
    assert counts["rows"] > 0 and counts["vector"] > 0 and counts["mfma"] > 0, out.stdout


def test_wide_run_fixtures_list_the_files_present():
    runs = os.path.join(ROOT, "tests", "golden", "runs_wide")
    summary = json.load(open(os.path.join(runs, "summary.json")))
    assert sorted(summary) == ["cage24_gcmc", "cage6_nvt"]
    assert sorted(d for d in os.listdir(runs) if os.path.isdir(os.path.join(runs, d))) == sorted(summary)
    for case, rec in summary.items():
        assert sorted(os.listdir(os.path.join(runs, case, "expected"))) == rec["files"], case
        assert sorted(os.listdir(os.path.join(runs, case, "inputs"))) == ["system.data", "system.inc", "system.maniac"], case
        assert rec["as_written"] == (case == "cage24_gcmc") and not rec["reservoir"]
        last = open(os.path.join(runs, case, "expected", "moves.dat")).read().strip().split("\n")[-1].split()
        assert last == rec["last_moves_record"], case
        for f in rec["files"]:
            assert os.path.getsize(os.path.join(runs, case, "expected", f)) < (1 << 20), (case, f)
