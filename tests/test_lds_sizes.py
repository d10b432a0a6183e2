"""CPU-only: the dynamic-LDS sizes of the reciprocal kernels have one home (csrc/mgpu_internal.h); a size that disagrees
with a kernel's layout is an out-of-bounds LDS access.  The expressions the launch sites carried before they were gathered
there are written out below, as they stood, and compared with the shared functions over everything an engine admits: kmax
1..32 per axis, the row count that goes with it, molecules of 1..400 sites, the row and per-k forms, both wide forms, one
tile and several."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
using namespace mgpu;
typedef struct { double x, y; } double2_;
typedef struct { int x, y, z, w; } int4_;

// ---- the expressions of the launch sites before this header held them
static size_t old_recip_lds_bytes(int ktot, int n1_max) { return (size_t)2 * n1_max * ktot * sizeof(double2_) + (size_t)n1_max * sizeof(double); }
static int old_recip_tile_sites(int ktot, int n1_max) {
    const size_t per_site = old_recip_lds_bytes(ktot, 1);
    return std::max(1, std::min(n1_max, (int)((size_t)(48 * 1024) / per_site)));
}
static size_t old_recip_rows_lds_bytes(int ktot, int n_rrows, int n1_max) {
    return old_recip_lds_bytes(ktot, n1_max) + (size_t)n_rrows * (2 * n1_max * sizeof(double2_));
}
static const size_t kOldWideTableBytes = 40 * 1024, kOldWideLdsBytes = 60 * 1024;
static int old_wide_rows_per_tile(int ktot, int n_rrows, int n1_max) {
    const size_t nss = (size_t)2 * n1_max;
    const size_t tables = nss * ktot * sizeof(double2_) + nss * sizeof(double);
    if (tables > kOldWideTableBytes) return 0;
    const int rpt = (int)((kOldWideLdsBytes - tables) / (nss * sizeof(double2_)));
    return rpt >= 8 ? std::min(rpt, n_rrows) : 0;
}
static int old_wide_mfma_tile(int ktot, int n_rrows, int n1_max) {
    const size_t nss = ((size_t)2 * n1_max + 3) & ~(size_t)3;
    const size_t per_ss = (size_t)ktot * sizeof(double2_) + sizeof(double), fixed = (size_t)n_rrows * sizeof(int4_);
    if (fixed + 4 * per_ss > kOldWideLdsBytes) return 0;
    const size_t fit = ((kOldWideLdsBytes - fixed) / per_ss) & ~(size_t)3;
    const size_t n_tiles = (nss + fit - 1) / fit;
    return (int)((((nss + n_tiles - 1) / n_tiles) + 3) & ~(size_t)3);
}
// launch_recip's wide launch
static size_t old_launch_wide_lds(int ktot, int n_rrows, int nss_max, int wide_rpt, bool wide_mfma) {
    return (size_t)nss_max * ktot * sizeof(double2_) + (size_t)wide_rpt * nss_max * sizeof(double2_) + (size_t)nss_max * sizeof(double) +
           (wide_mfma ? (size_t)n_rrows * sizeof(int4_) : 0);
}
// farm_type_form's two cases (behind kFarmKFront)
static size_t old_farm_vector_lds(size_t ktot, int nss, int rpt) {
    return (size_t)nss * ktot * sizeof(double2_) + (size_t)rpt * nss * sizeof(double2_) + (size_t)nss * sizeof(double);
}
static size_t old_farm_mfma_lds(size_t ktot, int n_rrows, int nss) {
    return (size_t)nss * ktot * sizeof(double2_) + (size_t)nss * sizeof(double) + (size_t)n_rrows * sizeof(int4_);
}

int main() {
    long long points = 0, bad = 0, tiled = 0, untiled = 0, vec = 0;
    for (int k0 = 1; k0 <= 32; ++k0)
        for (int k1 = 1; k1 <= 32; ++k1) {
            // rows (kx, ky) of the k list: kx = 0..kmax, ky = -kmax..kmax without the mirror half of kx = 0; the |k|^2 cut
            // of a real list leaves fewer: half of them as well
            const int full = (k0 + 1) * (2 * k1 + 1) - k1 - 1;
            for (int k2 = 1; k2 <= 32; ++k2) {
                const int kmax[3] = {k0, k1, k2};
                const int ktot = k0 + k1 + k2 + 3;
                bad += recip_ktot(kmax) != ktot;
                for (int n_rrows : {full, (full + 1) / 2})
                    for (int n1 = 1; n1 <= 400; ++n1) {
                        ++points;
                        bad += recip_lds_bytes(ktot, n1) != old_recip_lds_bytes(ktot, n1);
                        bad += recip_rows_lds_bytes(ktot, n_rrows, n1) != old_recip_rows_lds_bytes(ktot, n_rrows, n1);
                        const int tile = old_recip_tile_sites(ktot, n1);
                        bad += recip_tile_sites(ktot, n1) != tile;
                        bad += recip_lds_bytes(ktot, tile) != old_recip_lds_bytes(ktot, tile);
                        const int rpt = old_wide_rows_per_tile(ktot, n_rrows, n1);
                        bad += recip_wide_rows_per_tile(ktot, n_rrows, n1) != rpt;
                        if (rpt) {
                            ++vec;
                            bad += recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false) != old_launch_wide_lds(ktot, n_rrows, 2 * n1, rpt, false);
                            bad += recip_wide_lds_bytes(ktot, n_rrows, 2 * n1, rpt, false) != old_farm_vector_lds(ktot, 2 * n1, rpt);
                        }
                        const int mt = old_wide_mfma_tile(ktot, n_rrows, n1);
                        bad += recip_wide_mfma_tile(ktot, n_rrows, n1) != mt;
                        if (mt) {
                            (mt < ((2 * n1 + 3) & ~3) ? tiled : untiled) += 1;
                            bad += recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true) != old_launch_wide_lds(ktot, n_rrows, mt, 0, true);
                            bad += recip_wide_lds_bytes(ktot, n_rrows, mt, 0, true) != old_farm_mfma_lds(ktot, n_rrows, mt);
                        }
                    }
            }
        }
    std::printf("points %lld bad %lld vector %lld mfma_one_tile %lld mfma_tiled %lld\n", points, bad, vec, untiled, tiled);
    return bad != 0;
}
"""


def test_lds_sizes_equal_the_launch_sites_former_expressions(tmp_path):
    src = tmp_path / "lds_sizes.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "lds_sizes"
    # (any C++17 host compiler: the header is plain C++; hipcc is the one the build needs anyway)
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert out.returncode == 0 and fields[:1] == ["points"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert counts["points"] == 32 ** 3 * 2 * 400 and counts["bad"] == 0, out.stdout
    # every form was met, so that none of the comparisons above was vacuous
    assert counts["vector"] > 0 and counts["mfma_one_tile"] > 0 and counts["mfma_tiled"] > 0, out.stdout
