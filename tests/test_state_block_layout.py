"""CPU-only: the state block of mgpu_state_export_* / mgpu_state_import has one description, the integer functions of
csrc/mgpu_internal.h (state_rec_at, state_data_at, state_type_segments, ...), which the host code and -- through the item
table -- the kernel read.  They are compiled here without a device and held to a Python restatement of the layout as
include/maniac_gpu.h states it, over 1 to 3 residue types, n1 in {1, 3, 5, 24, 64}, counts in {0, 1, 63, 64, 65}, with and
without frames and reservoirs: the segments do not overlap, every segment and plane the 16-byte accesses may touch starts on
an even word, the total is as computed, and a header written with these functions reads back through the restatement."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N1S = (1, 3, 5, 24, 64)
COUNTS = (0, 1, 63, 64, 65)

# reads cases "n_res n_slots frames  (n1 cap n held rsv_cap) x n_res" for TWO listed replicas that share the counts except that
# the second holds one molecule less of its first type; prints, per case, the header words and the total
PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
using namespace mgpu;
int main() {
    int n_res, n_slots, frames;
    while (std::scanf("%d %d %d", &n_res, &n_slots, &frames) == 3) {
        int n1[3], cap[3], cnt[3], held[3], rsv[3];
        for (int t = 0; t < n_res; ++t) if (std::scanf("%d %d %d %d %d", &n1[t], &cap[t], &cnt[t], &held[t], &rsv[t]) != 5) return 2;
        const int n = 2;
        std::vector<long long> head(state_data_at(n, n_res), 0);
        head[0] = kStateMagic; head[1] = n; head[2] = n_res; head[3] = n_slots; head[4] = frames;
        for (int t = 0; t < n_res; ++t) { head[state_types_at() + 2 * t] = n1[t]; head[state_types_at() + 2 * t + 1] = cap[t]; }
        size_t at = state_data_at(n, n_res);
        for (int i = 0; i < n; ++i) {
            head[state_reps_at(n_res) + 2 * i] = 7 - i;
            head[state_reps_at(n_res) + 2 * i + 1] = (long long)at;
            at += state_A_words(n_slots);
            for (int t = 0; t < n_res; ++t) {
                const int nm = (i == 1 && t == 0 && cnt[t] > 0) ? cnt[t] - 1 : cnt[t];
                const int nf = frames ? state_frames_held(nm, held[t] != 0) : 0;
                const StateSegs s = state_type_segments(at, nm, nf, n1[t], rsv[t], frames != 0);
                long long *rec = &head[state_rec_at(n, n_res, i, t)];
                rec[kStateRecN] = nm; rec[kStateRecNf] = nf; rec[kStateRecRsvCap] = rsv[t]; rec[kStateRecFlags] = held[t] ? kStateFramesHeld : 0;
                rec[kStateRecPos] = s.pos; rec[kStateRecCom] = s.com; rec[kStateRecOff] = s.off; rec[kStateRecRsv] = s.rsv;
                at = s.end;
            }
        }
        head[5] = (long long)at;
        std::printf("%zu", head.size());
        for (long long v : head) std::printf(" %lld", v);
        // the vector rule at the four parities
        std::printf(" %d%d%d%d%d\n", (int)state_item_vec(2, 4, 6, 8), (int)state_item_vec(1, 4, 6, 8), (int)state_item_vec(2, 3, 6, 8),
                    (int)state_item_vec(2, 4, 5, 8), (int)state_item_vec(2, 4, 6, 7));
    }
    return 0;
}
"""

MAGIC = int.from_bytes(b"MMPUSTA1", "little")


def _up2(w):
    return (w + 1) & ~1


def _restated(n_res, n_slots, frames, types):
    """The layout in include/maniac_gpu.h's words, for the two listed replicas of PROGRAM: (header words, segments, total);
    segments = (first word, words, must be 16-byte aligned) of everything the data part holds."""
    n = 2
    types_at = 8 + 12
    reps_at = types_at + 2 * n_res
    recs_at = reps_at + 2 * n
    data_at = _up2(recs_at + 8 * n * n_res)
    head = [0] * data_at
    head[0:5] = [MAGIC, n, n_res, n_slots, frames]
    for t, (n1, cap, cnt, held, rsv) in enumerate(types):
        head[types_at + 2 * t: types_at + 2 * t + 2] = [n1, cap]
    at = data_at
    segs = []
    for i in range(n):
        head[reps_at + 2 * i: reps_at + 2 * i + 2] = [7 - i, at]
        segs.append((at, 2 * n_slots, True))
        at += 2 * n_slots
        for t, (n1, cap, cnt, held, rsv) in enumerate(types):
            nm = cnt - 1 if (i == 1 and t == 0 and cnt > 0) else cnt
            nf = (nm if nm > 0 else (1 if held else 0)) if frames else 0
            rec = [nm, nf, rsv, 8 if held else 0, at, -1, -1, -1]
            for d in range(3):
                segs.append((at + d * _up2(nm * n1), nm * n1, True))
            at += 3 * _up2(nm * n1)
            if frames:
                rec[5] = at
                for d in range(3):
                    segs.append((at + d * _up2(nf), nf, True))
                at += 3 * _up2(nf)
                rec[6] = at
                for d in range(3):
                    segs.append((at + d * _up2(nf * n1), nf * n1, True))
                at += 3 * _up2(nf * n1)
            if rsv > 0:
                rec[7] = at
                segs.append((at, 1, True))                      # {count, capacity}
                segs.append((at + 2, 3 * rsv * n1, True))       # the reservoir's block, behind a word of padding
                at += 2 + _up2(3 * rsv * n1)
            r0 = recs_at + 8 * (i * n_res + t)
            head[r0: r0 + 8] = rec
    head[5] = at
    return head, segs, at


def _cases():
    out = []
    for n_res in (1, 2, 3):
        for frames, with_rsv in itertools.product((0, 1), (0, 1)):
            # every (n1, count) pair in the first type; the others walk the grids so that every pair of neighbours occurs
            for a, (n1, cnt) in enumerate(itertools.product(N1S, COUNTS)):
                types = []
                for t in range(n_res):
                    n1_t = N1S[(N1S.index(n1) + t) % len(N1S)]
                    cnt_t = COUNTS[(COUNTS.index(cnt) + 2 * t) % len(COUNTS)]
                    held = 1 if (frames and (cnt_t > 0 or (a + t) % 2 == 0)) else 0
                    rsv = (cnt_t + 66 + 5 + t) if (with_rsv and t != 1) else 0
                    types.append((n1_t, 66, cnt_t, held, rsv))
                out.append((n_res, 3 + 2 * a, frames, types))
    return out


def test_state_block_layout_is_the_stated_one(tmp_path):
    src = tmp_path / "state_layout.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "state_layout"
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    cases = _cases()
    text = "".join(f"{n_res} {n_slots} {frames} " + " ".join(" ".join(map(str, ty)) for ty in types) + "\n"
                   for n_res, n_slots, frames, types in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(cases) == 3 * 4 * 25
    met = set()
    for (n_res, n_slots, frames, types), line in zip(cases, lines):
        f = line.split()
        n_head = int(f[0])
        got = [int(v) for v in f[1: 1 + n_head]]
        assert f[1 + n_head] == "10000", "16-byte accesses only where block offset, engine offset, length and stride are even"
        head, segs, total = _restated(n_res, n_slots, frames, types)
        assert got == head, (n_res, n_slots, frames, types, [(i, a, b) for i, (a, b) in enumerate(zip(got, head)) if a != b][:4])
        assert got[5] == total and total % 2 == 0
        # no overlap: in the order laid out, every segment starts at or behind the end of the one before and inside the block
        end = n_head
        for at, words, aligned in segs:
            assert at >= end and at + words <= total, (at, words, end, total)
            assert not aligned or at % 2 == 0, (at, words)
            end = at + words
        # round trip: the records read back give the counts that went in
        for i in range(2):
            for t, (n1, cap, cnt, held, rsv) in enumerate(types):
                rec = got[8 + 12 + 2 * n_res + 4 + 8 * (i * n_res + t):][:8]
                nm = cnt - 1 if (i == 1 and t == 0 and cnt > 0) else cnt
                assert rec[0] == nm and rec[2] == rsv and (rec[3] == 8) == bool(held)
                assert (rec[5] >= 0) == (rec[6] >= 0) == bool(frames) and (rec[7] >= 0) == (rsv > 0)
                met.add((n1, nm, bool(frames), rsv > 0, rec[1] > nm))
    # every n1, every count, frames and reservoirs on and off, and the stale slot-0 frame of an empty type were met
    assert {m[0] for m in met} == set(N1S) and set(COUNTS) <= {m[1] for m in met}
    assert {m[2] for m in met} == {False, True} and {m[3] for m in met} == {False, True} and any(m[4] for m in met)
