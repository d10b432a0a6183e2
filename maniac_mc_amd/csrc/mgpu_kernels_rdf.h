// Radial distribution functions of MANY replicas per pass (mgpu_rdf_accumulate_replicas): one sample of a replica bins the
// minimum-image distance of every unordered pair of occupied atom slots whose atom types form a selected pair.  The counts are
// INTEGERS: a sum of ones does not depend on the order it is taken in, on the grid, on the replicas that share a launch or on
// the number of j chunks -- which is why this kernel may add with atomics where the energy paths may not.
//
// Grid (tile, replica of the pass), 256 threads.  A tile = (i block of 256 atom slots, j chunk).  The i block's coordinates,
// atom types and molecule keys are staged once in LDS; every thread then owns one j slot at a time (j >= the block's first
// slot; j > i inside the diagonal group) and walks the i block, whose reads are LDS broadcasts.  The pair table -- (atom type,
// atom type) -> index of the selected pair, a nibble per entry, 0xF: none -- is looked up in the j lane's own packed row BEFORE
// any distance arithmetic; an i block, or a wave's 64 j slots, none of whose atom types has a selected partner on the other
// side is skipped by a uniform test (a framework pays nothing for framework-framework pairs when only guest-framework is
// wanted).  Bins are added with LDS atomics into the workgroup's histogram unsigned[n_pairs][n_bins] (at most 32 KiB); the
// eligible pairs are counted in registers; at the end the workgroup adds its non-zero bins to the replica's 64-bit
// accumulators in HBM with vector atomics.
#ifndef MGPU_KERNELS_RDF_H
#define MGPU_KERNELS_RDF_H

#include "mgpu_kernels_common.h"

namespace mgpu {

constexpr int kRdfBlock = 256;        // threads per workgroup = atom slots of an i block = j slots of a group
constexpr int kRdfMaxPairs = 8;       // selected atom-type pairs (a nibble each in the packed rows; 8 x 1024 bins x 4 B = 32 KiB)
constexpr int kRdfMaxBins = 1024;
constexpr int kRdfNone = 0xF;         // packed-row entry: the two atom types form no selected pair

// the engine's device copy of the selection: row[a] = the pair indices of (a, b), b = 0 .. 15, a nibble each (kRdfNone: none);
// partner[a] = the atom types b that form a selected pair with a, a bit each
struct RdfTable {
    unsigned long long row[kMaxTypes];
    unsigned partner[kMaxTypes];
};

struct RdfArgs {
    int n_bins, n_pairs, include_intra;
    int n_chunk;                      // j chunks per i block: group g of an i block belongs to chunk g % n_chunk
    double r_max2, inv_dr;            // r_max * r_max and n_bins / r_max, formed once on the host
};

// acc = hist [R][n_pairs][n_bins] | eligible [R][n_pairs] | samples [R]
template <bool TRI>
static __global__ __launch_bounds__(kRdfBlock) void rdf_hist_kernel(Topo tp, BoxDev bx, RdfArgs ra, const double *__restrict__ pos,
                                                                    const int *__restrict__ nmol, const int *__restrict__ atom_res,
                                                                    const int *__restrict__ atom_mol, const int *__restrict__ reps,
                                                                    const RdfTable *__restrict__ tab, unsigned long long *__restrict__ hist,
                                                                    unsigned long long *__restrict__ eligible,
                                                                    unsigned long long *__restrict__ samples) {
    extern __shared__ unsigned s_hist[];                       // [n_pairs][n_bins]
    __shared__ double s_x[kRdfBlock], s_y[kRdfBlock], s_z[kRdfBlock];
    __shared__ int s_ty[kRdfBlock], s_key[kRdfBlock];          // atom type (-1: unoccupied or without a selected partner), molecule key
    __shared__ unsigned long long s_row[kMaxTypes];
    __shared__ unsigned s_partner[kMaxTypes];
    __shared__ unsigned long long s_elig[kRdfMaxPairs];
    __shared__ unsigned s_imask;

    const int tid = threadIdx.x;
    const int replica = reps[blockIdx.y];
    const int ib = blockIdx.x / ra.n_chunk, chunk = blockIdx.x % ra.n_chunk;
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&samples[replica], 1ull);
    const int ncap = tp.n_cap_atoms;
    const int i0 = ib * kRdfBlock;
    const int n_groups = (ncap - i0 + kRdfBlock - 1) / kRdfBlock;       // j groups of this i block: slots i0 + g * 256 ...
    if (chunk >= n_groups) return;                                      // (uniform) a chunk without a group
    const int n_hist = ra.n_pairs * ra.n_bins;
    const int *cnt = nmol + (size_t)replica * tp.n_res;
    const double *px = pos + (size_t)replica * 3 * ncap, *py = px + ncap, *pz = py + ncap;

    if (tid < kMaxTypes) { s_row[tid] = tab->row[tid]; s_partner[tid] = tab->partner[tid]; }
    if (tid < kRdfMaxPairs) s_elig[tid] = 0;
    if (tid == 0) s_imask = 0;
    for (int b = tid; b < n_hist; b += kRdfBlock) s_hist[b] = 0;
    __syncthreads();
    {
        const int i = i0 + tid;
        int ty = -1, key = -1;
        double x = 0.0, y = 0.0, z = 0.0;
        if (i < ncap) {
            const int res = atom_res[i], mol = atom_mol[i];
            if (mol < cnt[res]) {
                const int t = tp.slot_ty[i];
                if (s_partner[t]) {
                    ty = t;
                    if (!ra.include_intra) key = (res << 28) | mol;     // (with intramolecular pairs: -1, no j has that key)
                    x = px[i]; y = py[i]; z = pz[i];
                }
            }
        }
        s_x[tid] = x; s_y[tid] = y; s_z[tid] = z; s_ty[tid] = ty; s_key[tid] = key;
        if (ty >= 0) atomicOr(&s_imask, 1u << ty);
    }
    __syncthreads();
    const unsigned imask = s_imask;
    if (imask == 0) return;                                             // (uniform) nothing in this i block can form a selected pair

    unsigned elig[kRdfMaxPairs];
#pragma unroll
    for (int q = 0; q < kRdfMaxPairs; ++q) elig[q] = 0;
    for (int g = chunk; g < n_groups; g += ra.n_chunk) {
        const int j = i0 + g * kRdfBlock + tid;
        unsigned want = 0;
        int tj = -1, keyj = 0;
        if (j < ncap) {
            const int res = atom_res[j], mol = atom_mol[j];
            if (mol < cnt[res]) {
                tj = tp.slot_ty[j];
                want = s_partner[tj] & imask;
                keyj = (res << 28) | mol;
            }
        }
        if (__ballot(want != 0) == 0) continue;                         // (per wave) these 64 j slots have no partner in the i block
        unsigned long long rowj = ~0ull;                                // every nibble kRdfNone
        double xj = 0.0, yj = 0.0, zj = 0.0;
        if (want) { rowj = s_row[tj]; xj = px[j]; yj = py[j]; zj = pz[j]; }
        // the diagonal group holds the i block itself: i < j there is (local i) < tid, and the wave stops at its last lane
        const int i_lim = g == 0 ? tid : kRdfBlock;
        const int i_end = g == 0 ? min(kRdfBlock, (tid | 63) + 1) : kRdfBlock;
        for (int h0 = 0; h0 < i_end; h0 += 128) {
            unsigned long long packed = 0;                              // eight 8-bit counts: at most 128 each before they are unpacked
            const int h1 = min(i_end, h0 + 128);
            for (int ii = h0; ii < h1; ++ii) {
                const int ti = __builtin_amdgcn_readfirstlane(s_ty[ii]);
                if (ti < 0) continue;
                const int p = (int)(rowj >> (4 * ti)) & kRdfNone;
                if (p != kRdfNone && ii < i_lim && s_key[ii] != keyj) {
                    packed += 1ull << (8 * p);
                    const double r2 = image_r2<TRI>(xj - s_x[ii], yj - s_y[ii], zj - s_z[ii], bx);
                    if (r2 < ra.r_max2) {
                        const int b = (int)(sqrt(r2) * ra.inv_dr);
                        if (b < ra.n_bins) atomicAdd(&s_hist[p * ra.n_bins + b], 1u);   // b == n_bins: rounding at the top edge, dropped
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < kRdfMaxPairs; ++q) elig[q] += (unsigned)(packed >> (8 * q)) & 0xffu;
        }
    }
#pragma unroll
    for (int q = 0; q < kRdfMaxPairs; ++q)
        if (elig[q]) atomicAdd(&s_elig[q], (unsigned long long)elig[q]);
    __syncthreads();
    unsigned long long *h = hist + (size_t)replica * n_hist;
    for (int b = tid; b < n_hist; b += kRdfBlock) {
        const unsigned v = s_hist[b];
        if (v) atomicAdd(&h[b], (unsigned long long)v);
    }
    if (tid < ra.n_pairs && s_elig[tid]) atomicAdd(&eligible[(size_t)replica * ra.n_pairs + tid], s_elig[tid]);
}

}  // namespace mgpu

#endif
