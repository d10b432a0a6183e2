"""CPU-only: the two blocks of a batched trial on a lane -- the pinned staging block and the result block -- have one
description (csrc/mgpu_internal.h: trial_staging, trial_result, lane_site_buffer_bytes).  A block that disagrees between
its writer and a reader gives a wrong energy, not a crash.  The expressions trial_submit_impl, trial_wait_impl and
mgpu_lane_site_buffer carried before the layouts were gathered there are written out below, as they stood, and compared
with the shared functions over every trial shape a lane admits: 1..4097 candidates, rows of 1..64 sites, host-built and
device-built rows, with and without the reservoir pick, the deciding form, the framework's extra records, 1..32 splits,
fused and single segments.  The size mgpu_lane_site_buffer reserves is also held to what it promises: it covers every
staging layout of at most n_max candidates of at most site_stride sites (the former expression's margins were added by
hand and never checked)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
using namespace mgpu;
// the records of the blocks, member for member (mgpu_kernels_common.h, mgpu_kernels_recip.h)
struct PairItem { int replica, t, m, src, ordered; };
struct RecipItem { int replica, t, m, kind, src, aux, frame; };
struct DecideItem { int old_off, old_stride, old_ns, old_extra, new_off, new_stride, new_ns, new_extra, intra, kind; double self, pref, u; };

// ---- the expressions of trial_submit_impl before this header held them
struct OldStaging { int site_stride, frame_at, pick_at; size_t site_bytes, pit, rit, iit, iit_end, build_at, build_u, dec_at, total; };
static OldStaging old_staging(int n, int site_stride, bool build, bool rsv_any, bool decide) {
    OldStaging o{};
    if (build) {
        const int n1_all = site_stride;
        o.frame_at = n1_all;
        site_stride = 2 * n1_all + 1 + (rsv_any ? 1 : 0);
        o.pick_at = rsv_any ? 2 * o.frame_at + 1 : 0;
    }
    o.site_stride = site_stride;
    const size_t site_bytes = (size_t)n * site_stride * 3 * sizeof(double);
    const size_t pit_cap = 2 * (size_t)n * sizeof(PairItem), rit_bytes = (size_t)n * sizeof(RecipItem);
    const size_t iit_cap = (size_t)n * sizeof(PairItem);
    const size_t build_at = (site_bytes + pit_cap + rit_bytes + iit_cap + 7) & ~(size_t)7;
    const size_t build_mv = ((size_t)n * sizeof(int) + 7) & ~(size_t)7;
    const size_t build_bytes = build ? build_mv + (size_t)5 * n * sizeof(double) : 0;
    const size_t dec_at = (build_at + build_bytes + 7) & ~(size_t)7;
    const size_t dec_bytes = decide ? (size_t)n * sizeof(DecideItem) : 0;
    o.site_bytes = site_bytes;
    o.pit = site_bytes;
    o.rit = site_bytes + pit_cap;
    o.iit = site_bytes + pit_cap + rit_bytes;
    o.iit_end = site_bytes + pit_cap + rit_bytes + iit_cap;      // the in-place rows' first bound
    o.build_at = build_at;
    o.build_u = build_at + build_mv;
    o.dec_at = dec_at;
    o.total = dec_at + dec_bytes;
    return o;
}
// ---- of mgpu_lane_site_buffer
static size_t old_trial_staging_bytes(int n, int site_stride) {
    return (size_t)n * site_stride * 3 * sizeof(double) + 2 * (size_t)n * sizeof(PairItem) + (size_t)n * sizeof(RecipItem) +
           (size_t)n * sizeof(PairItem) + 16 + (size_t)n * sizeof(DecideItem);
}
static size_t old_lane_site_buffer(int n_max, int site_stride) {
    const size_t built = old_trial_staging_bytes(n_max, 2 * site_stride + 2) + ((size_t)n_max * sizeof(int) + 8) + (size_t)5 * n_max * sizeof(double) + 16;
    return std::max(old_trial_staging_bytes(n_max, site_stride), built);
}

static TrialStaging staging(int n, int s, bool built, bool pick, bool decide) {
    return trial_staging<sizeof(PairItem), sizeof(RecipItem), sizeof(DecideItem)>(n, s, built, pick, decide);
}

int main() {
    long long bad = 0, unsound = 0, staged[8] = {0}, lent = 0, results[2][2][4] = {{{0}}};
    for (int n = 1; n <= 4097; ++n)
        for (int s = 1; s <= 64; ++s) {
            for (int v = 0; v < 8; ++v) {
                const bool built = v & 1, pick = v & 2, decide = v & 4;
                const OldStaging o = old_staging(n, s, built, pick, decide);
                const TrialStaging a = staging(n, s, built, pick, decide);
                ++staged[v];
                bad += a.row_sites != o.site_stride || a.frame_at != o.frame_at || a.pick_at != o.pick_at;
                bad += a.sites != 0 || a.pair_items != o.pit || a.k_items != o.rit || a.intra_items != o.iit;
                bad += a.moves != o.build_at || a.moves != o.iit_end;
                bad += built && a.uniforms != o.build_u;
                bad += a.decide_items != o.dec_at || a.total != o.total;
            }
            // the lent block: the former value, and enough for every shape it is promised for -- the shapes at and just
            // below (n, s) and the smallest, and no layout shrinks as n or the site count grows
            const size_t lend = lane_site_buffer_bytes<sizeof(PairItem), sizeof(RecipItem), sizeof(DecideItem)>(n, s);
            ++lent;
            bad += lend != old_lane_site_buffer(n, s);
            for (int v = 0; v < 8; ++v) {
                const bool built = v & 1, pick = v & 2, decide = v & 4;
                const size_t here = staging(n, s, built, pick, decide).total;
                for (int nn : {n, std::max(1, n - 1), 1})
                    for (int n1 : {s, std::max(1, s - 1), 1}) unsound += staging(nn, n1, built, pick, decide).total > lend;
                unsound += staging(n + 1, s, built, pick, decide).total < here || staging(n, s + 1, built, pick, decide).total < here;
            }
        }
    // the result block: n_partials and n_pair as the segments of trial_submit_impl give them -- fused moves (two entries
    // per item), single-state moves (two items), insertions / deletions (one item), or half fused moves and half
    // insertions; nsplit partial records per entry, none where the framework sweep's extra record is all (nsplit 0)
    for (int n = 1; n <= 4097; ++n)
        for (int nsplit = 0; nsplit <= 32; ++nsplit)
            for (int shape = 0; shape < 4; ++shape)
                for (int v = 0; v < 4; ++v) {
                    const bool frozen_extra = v & 1, decide = v & 2;
                    if (nsplit == 0 && !frozen_extra) continue;
                    const int n_moves = shape == 3 ? n / 2 : 0;
                    const int n_pair = shape < 2 ? 2 * n : (shape == 2 ? n : 2 * n_moves + (n - n_moves));
                    const int n_partials = n_pair * nsplit;
                    // trial_submit_impl
                    const size_t extra_at = 2 * (size_t)n_partials + 3 * (size_t)n;
                    const size_t acc_at = extra_at + (frozen_extra ? 2 * (size_t)n_pair : 0);
                    const size_t out_doubles = acc_at + (decide ? ((size_t)n + 1) / 2 : 0);
                    const size_t d_uo = 2 * (size_t)n_partials, d_un = d_uo + n, d_in = d_un + n;
                    const size_t decided_at = acc_at * sizeof(double);
                    // trial_wait_impl
                    const size_t uo = 2 * (size_t)n_partials, un = uo + n, in = un + n, ex = in + n;
                    const TrialResult r = trial_result(n, n_partials, n_pair, frozen_extra, decide);
                    ++results[frozen_extra][decide][shape];
                    bad += r.partials != 0 || r.u_old != d_uo || r.u_new != d_un || r.intra != d_in || r.extra != extra_at;
                    bad += r.u_old != uo || r.u_new != un || r.intra != in || r.extra != ex;
                    bad += r.flags != acc_at || r.flags_bytes() != decided_at || r.total != out_doubles;
                }
    std::printf("bad %lld unsound %lld lent %lld", bad, unsound, lent);
    for (int v = 0; v < 8; ++v) std::printf(" staging_%s_%s_%s %lld", v & 1 ? "built" : "host", v & 2 ? "pick" : "nopick", v & 4 ? "decide" : "plain", staged[v]);
    for (int f = 0; f < 2; ++f)
        for (int d = 0; d < 2; ++d)
            for (int sh = 0; sh < 4; ++sh) std::printf(" result_%s_%s_shape%d %lld", f ? "extra" : "noextra", d ? "decide" : "plain", sh, results[f][d][sh]);
    std::printf("\n");
    return bad != 0 || unsound != 0;
}
"""


def test_trial_layouts_equal_the_former_expressions_and_the_lent_block_suffices(tmp_path):
    src = tmp_path / "trial_layout.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "trial_layout"
    # (any C++17 host compiler: the header is plain C++; hipcc is the one the build needs anyway)
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert fields[:1] == ["bad"], out.stdout + out.stderr
    counts = dict(zip(fields[0::2], map(int, fields[1::2])))
    assert out.returncode == 0 and counts["bad"] == 0 and counts["unsound"] == 0, out.stdout
    # every variant was met, so that none of the comparisons above was vacuous
    assert len(counts) == 3 + 8 + 16 and all(v > 0 for k, v in counts.items() if k not in ("bad", "unsound")), out.stdout
    assert counts["lent"] == 4097 * 64 and counts["staging_built_pick_decide"] == 4097 * 64, out.stdout
