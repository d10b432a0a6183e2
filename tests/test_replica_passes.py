"""CPU-only: what the farm analyses of csrc/mgpu_replicas.hip share has its arithmetic in csrc/mgpu_internal.h -- plan_passes (the
passes of mgpu_system_energy_replicas and mgpu_energy_pairs_replicas), Accum / accum_layout (the accumulators of rdf and density)
and nibble_get / nibble_set (their packed type tables).  The expressions the entry points carried before are written out below
as they stood -- the pass loop, rdf_blocks, density_blocks and the shift-and-mask lines of the two configure calls -- and compared
with the shared functions:

* passes: lists of 0..40 replicas with n_pair drawn from {0, 1, 7, 2^20, 2^27} and n_in from [0, n_pair], chunk in {0, 1, 3, 40,
  40000}, nsplit in {1, 8, 64}, a replica's bytes a + 48 n_pair + 32 n_in with a from 1 KiB to 300 MiB (beyond the pass budget:
  the replica still gets its pass); first, count, n_pair and n_in of every pass and the refusal at 2^31 work units (reached by
  2^27 items at 64 splits);
* accumulators: R = 1..5 entries, 1..8 pairs x 1..1024 bins (rdf), 1..8 channels x grids up to 4 x 3 x 2 (density): the word of
  every segment of every entry and the block's bytes;
* nibbles: get and set of every slot 0..15 with every value 0..15 on full and partly filled words, and whole tables built from
  lists of pairs and of channels with every type 0..15, duplicates included."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mgpu_internal.h"
#include <cstdio>
#include <vector>
using namespace mgpu;

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned long long rnd() {                       // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}

// ---- the pass loop as mgpu_system_energy_replicas and mgpu_energy_pairs_replicas both carried it
static const size_t kOldPassBytes = (size_t)256 << 20;
static const int kOldPassMax = 32768, kPairWaves = 8;
static const long long kOldPassItems = (long long)1 << 28;
struct Rep { long long n_pair, n_in; };
template <class BytesOf>
static bool old_passes(int n, const Rep *reps, BytesOf bytes_of, int chunk, int nsplit, std::vector<Pass> &passes) {
    const int most = chunk > 0 ? std::min(chunk, kOldPassMax) : kOldPassMax;
    for (int i = 0; i < n;) {
        Pass p{i, 0, 0, 0};
        size_t bytes = 0;
        while (i < n && p.c < most) {
            long long np, ni;
            np = reps[i].n_pair; ni = reps[i].n_in;
            const size_t b = bytes_of(np, ni);
            if (p.c > 0 && (bytes + b > kOldPassBytes || (p.n_pair + np) * nsplit > kOldPassItems)) break;
            bytes += b; p.n_pair += np; p.n_in += ni; p.c += 1; ++i;
        }
        if (p.n_pair * nsplit >= ((long long)1 << 31) - kPairWaves) return false;
        passes.push_back(p);
    }
    return true;
}

static long long pass_cases, pass_bad, pass_refused, pass_planned, pass_alone_over, pass_many;
static void pass_case(int n, int chunk, int nsplit, size_t a, bool no_giant) {
    static const long long kinds[5] = {0, 1, 7, 1ll << 20, 1ll << 27};
    std::vector<Rep> reps(n);
    for (Rep &r : reps) {
        r.n_pair = kinds[rnd() % (no_giant ? 4 : 5)];
        r.n_in = r.n_pair ? (long long)(rnd() % (unsigned long long)(r.n_pair + 1)) : 0;
    }
    auto bytes_of = [&](long long np, long long ni) { return a + (size_t)np * 48 + (size_t)ni * 32; };
    std::vector<Pass> was, is;
    const bool was_ok = old_passes(n, reps.data(), bytes_of, chunk, nsplit, was);
    const bool is_ok = plan_passes(n, [&](int i, long long &np, long long &ni) { np = reps[i].n_pair; ni = reps[i].n_in; }, bytes_of,
                                   chunk, nsplit, is);
    ++pass_cases;
    if (was_ok != is_ok) { ++pass_bad; return; }
    if (!was_ok) { ++pass_refused; pass_bad += !is.empty(); return; }
    ++pass_planned;
    if (was.size() != is.size()) { ++pass_bad; return; }
    for (size_t k = 0; k < was.size(); ++k) {
        pass_bad += was[k].first != is[k].first || was[k].c != is[k].c || was[k].n_pair != is[k].n_pair || was[k].n_in != is[k].n_in;
        if (was[k].c == 1 && bytes_of(was[k].n_pair, was[k].n_in) > kOldPassBytes) ++pass_alone_over;
        if (was[k].c > 1) ++pass_many;
    }
}

// ---- rdf_blocks and density_blocks as they stood, in words from the start of d_acc
static long long acc_points, acc_bad;
static void rdf_case(size_t R, size_t n_pairs, size_t n_bins) {
    const size_t per = n_pairs * n_bins;
    const size_t hist = 0, eligible = hist + R * per, samples = eligible + R * n_pairs;
    const size_t bytes = (R * per + R * n_pairs + R) * sizeof(unsigned long long);
    const Accum a = accum_layout(R, n_pairs * n_bins, n_pairs, 1);
    acc_bad += a.n_seg != 3 || a.bytes() != bytes || a.per[0] != per || a.per[1] != n_pairs || a.per[2] != 1 || a.entries != R;
    acc_bad += a.at[0] != hist || a.at[1] != eligible || a.at[2] != samples;
    for (size_t r = 0; r < R; ++r, ++acc_points)
        acc_bad += a.word(0, r) != hist + r * per || a.word(1, r) != eligible + r * n_pairs || a.word(2, r) != samples + r;
}
static void density_case(size_t n_groups, size_t n_channels, size_t n0, size_t n1, size_t n2) {
    const size_t per_group = n_channels * n0 * n1 * n2, voxels = n0 * n1 * n2;
    const size_t hist = 0, samples = hist + n_groups * per_group;
    const unsigned long long bytes = ((unsigned long long)n_groups * n_channels * voxels + n_groups) * sizeof(unsigned long long);
    const Accum a = accum_layout(n_groups, n_channels * voxels, 1);
    acc_bad += a.n_seg != 2 || a.bytes() != bytes || a.per[0] != per_group || a.per[1] != 1 || a.entries != n_groups;
    acc_bad += a.at[0] != hist || a.at[1] != samples;
    for (size_t g = 0; g < n_groups; ++g, ++acc_points) acc_bad += a.word(0, g) != hist + g * per_group || a.word(1, g) != samples + g;
}

// ---- the nibble lines of mgpu_rdf_configure and mgpu_density_configure as they stood
static const int kRdfNone = 0xF, kDensityNone = 0xF, kMaxTypes = 16;
static long long nib_points, nib_bad, nib_duplicates;
static void nibble_word(unsigned long long w) {
    for (int slot = 0; slot < 16; ++slot) {
        nib_bad += (unsigned)((w >> (4 * slot)) & kRdfNone) != nibble_get(w, slot);
        for (unsigned v = 0; v < 16; ++v, ++nib_points) {
            const unsigned long long was = (w & ~((unsigned long long)kRdfNone << (4 * slot))) | ((unsigned long long)v << (4 * slot));
            nib_bad += was != nibble_set(w, slot, v) || nibble_get(was, slot) != v;
        }
    }
}
struct Table { unsigned long long row[kMaxTypes]; unsigned partner[kMaxTypes]; };
static void rdf_table(int n_pairs) {
    Table was, is;
    for (int a = 0; a < kMaxTypes; ++a) { was.row[a] = is.row[a] = ~0ull; was.partner[a] = is.partner[a] = 0; }
    for (int p = 0; p < n_pairs; ++p, ++nib_points) {
        const int a = (int)(rnd() % 16), b = (int)(rnd() % 16);
        const bool was_dup = ((was.row[a] >> (4 * b)) & kRdfNone) != (unsigned)kRdfNone;
        nib_bad += was_dup != (nibble_get(is.row[a], b) != kNibbleNone);
        if (was_dup) { ++nib_duplicates; continue; }
        was.row[a] = (was.row[a] & ~((unsigned long long)kRdfNone << (4 * b))) | ((unsigned long long)p << (4 * b));
        was.row[b] = (was.row[b] & ~((unsigned long long)kRdfNone << (4 * a))) | ((unsigned long long)p << (4 * a));
        is.row[a] = nibble_set(is.row[a], b, (unsigned)p);
        is.row[b] = nibble_set(is.row[b], a, (unsigned)p);
    }
    for (int a = 0; a < kMaxTypes; ++a) nib_bad += was.row[a] != is.row[a];
}
static void density_table(int n_channels) {
    unsigned long long was = ~0ull, is = ~0ull;
    for (int c = 0; c < n_channels; ++c, ++nib_points) {
        const int t = (int)(rnd() % 16);
        const bool was_dup = ((was >> (4 * t)) & kDensityNone) != (unsigned)kDensityNone;
        nib_bad += was_dup != (nibble_get(is, t) != kNibbleNone);
        if (was_dup) { ++nib_duplicates; continue; }
        was = (was & ~((unsigned long long)kDensityNone << (4 * t))) | ((unsigned long long)c << (4 * t));
        is = nibble_set(is, t, (unsigned)c);
    }
    nib_bad += was != is;
}

int main() {
    const int chunks[5] = {0, 1, 3, 40, 40000}, nsplits[3] = {1, 8, 64};
    const size_t sizes[6] = {(size_t)1 << 10, (size_t)64 << 10, (size_t)1 << 20, (size_t)20 << 20, (size_t)100 << 20, (size_t)300 << 20};
    for (int chunk : chunks)
        for (int nsplit : nsplits)
            for (int n = 0; n <= 40; ++n)
                for (size_t a : sizes)
                    for (int draw = 0; draw < 12; ++draw) pass_case(n, chunk, nsplit, a, draw % 3 == 0);
    pass_bad += kReplicasPassBytes != kOldPassBytes || kReplicasPassMax != kOldPassMax || kReplicasPassItems != kOldPassItems;
    for (size_t R = 1; R <= 5; ++R)
        for (size_t np = 1; np <= 8; ++np)
            for (size_t nb = 1; nb <= 1024; ++nb) rdf_case(R, np, nb);
    for (size_t G = 1; G <= 5; ++G)
        for (size_t nc = 1; nc <= 8; ++nc)
            for (size_t n0 = 1; n0 <= 4; ++n0)
                for (size_t n1 = 1; n1 <= 3; ++n1)
                    for (size_t n2 = 1; n2 <= 2; ++n2) density_case(G, nc, n0, n1, n2);
    nibble_word(~0ull);
    nibble_word(0);
    for (int k = 0; k < 64; ++k) nibble_word(rnd() | (k % 2 ? 0xF0F0F0F00F0F0F0Full : 0));
    for (int k = 0; k < 2000; ++k) { rdf_table(1 + k % 8); density_table(1 + k % 8); }
    nib_bad += kNibbleNone != (unsigned)kRdfNone;
    std::printf("pass_cases %lld pass_bad %lld pass_refused %lld pass_planned %lld pass_alone_over %lld pass_many %lld "
                "acc_points %lld acc_bad %lld nib_points %lld nib_bad %lld nib_duplicates %lld\n",
                pass_cases, pass_bad, pass_refused, pass_planned, pass_alone_over, pass_many, acc_points, acc_bad, nib_points, nib_bad,
                nib_duplicates);
    return pass_bad != 0 || acc_bad != 0 || nib_bad != 0;
}
"""


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    d = tmp_path_factory.mktemp("replica_passes")
    src, exe = d / "replica_passes.cpp", d / "replica_passes"
    src.write_text(PROGRAM)
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["hipcc", "-x", "c++"]
    subprocess.check_call(cxx + ["-std=c++17", "-O2", "-I", os.path.join(ROOT, "maniac_mc_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    fields = out.stdout.split()
    assert fields[:1] == ["pass_cases"], out.stdout + out.stderr
    return dict(zip(fields[0::2], map(int, fields[1::2])))


def test_plan_passes_equals_the_two_entry_points_former_loop(counts):
    assert counts["pass_cases"] > 0 and counts["pass_bad"] == 0, counts
    # the refusal, a replica beyond the byte budget in a pass of its own, and passes of several replicas were all met
    for key in ("pass_refused", "pass_planned", "pass_alone_over", "pass_many"):
        assert counts[key] > 0, (key, counts)


def test_accumulator_layout_and_nibbles_equal_the_former_expressions(counts):
    assert counts["acc_points"] > 0 and counts["acc_bad"] == 0, counts
    assert counts["nib_points"] > 0 and counts["nib_bad"] == 0 and counts["nib_duplicates"] > 0, counts
