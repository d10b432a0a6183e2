// Density maps of MANY replicas per pass (mgpu_density_accumulate_replicas): one sample of a replica adds every occupied atom
// slot whose atom type is a selected channel to the voxel of its fractional coordinates, folded into the cell.  The counts are
// INTEGERS: a sum of ones does not depend on the order it is taken in, on the grid, or on the replicas that share a launch or a
// map -- which is why this kernel may add with atomics where the energy paths may not.
//
// Grid (block of 256 atom slots, replica of the pass), one slot per thread.  The type -> channel table (a nibble per atom type,
// 0xF: none) is one 64-bit kernel argument and is looked up BEFORE any arithmetic; a wave none of whose 64 slots has a channel
// leaves by a ballot (a framework that was not asked for costs its slot-type loads and nothing else).  What is left forms the
// fractional coordinates of ApplyPBC, s = box%reciprocal (r - bounds_lo) (orthorhombic: (r_d - lo_d) invL_d), the voxel
// v_d = floor(s_d n_d) mod n_d (Euclidean: any number of cells away folds back, so v_d is in [0, n_d) whatever the coordinate
// holds) and adds 1 to the group's map with one 64-bit vector atomic in HBM.  The stream orders the passes.
#ifndef MGPU_KERNELS_DENSITY_H
#define MGPU_KERNELS_DENSITY_H

#include "mgpu_kernels_common.h"

namespace mgpu {

constexpr int kDensityBlock = 256;            // threads per workgroup = atom slots of a block
constexpr int kDensityMaxChannels = 8;        // selected atom types (a nibble each in the packed table)
constexpr int kDensityMaxAxis = 1024;         // voxels along one cell vector
constexpr long long kDensityMaxVoxels = 1ll << 24;                    // voxels of one map
constexpr int kDensityNone = 0xF;             // packed-table entry: the atom type is no channel

struct DensityArgs {
    int n[3];                         // voxels along the three cell vectors
    int n_channels;
    unsigned long long table;         // channel of atom type t = (table >> 4 t) & 0xF
};

// one coordinate's voxel: floor(u) mod n, Euclidean.  A u that no 64-bit integer holds (or a NaN) counts as 0, so the result
// is in [0, n) for every double.
__device__ __forceinline__ int density_voxel(double s, int n) {
    double u = floor(s * (double)n);
    if (!(fabs(u) < 0x1p62)) u = 0.0;
    const long long i = (long long)u;
    const int v = (int)(i % n);
    return v < 0 ? v + n : v;
}

// hist [n_groups][n_channels][n2][n1][n0], samples [n_groups]; group_of [R]: the map of every replica, -1: never counted
template <bool TRI>
static __global__ __launch_bounds__(kDensityBlock) void density_map_kernel(Topo tp, BoxDev bx, DensityArgs da, const double *__restrict__ pos,
                                                                           const int *__restrict__ nmol, const int *__restrict__ atom_res,
                                                                           const int *__restrict__ atom_mol, const int *__restrict__ reps,
                                                                           const int *__restrict__ group_of, unsigned long long *__restrict__ hist,
                                                                           unsigned long long *__restrict__ samples) {
    const int replica = reps[blockIdx.y];
    const int g = group_of[replica];
    if (g < 0) return;                                                  // (uniform) a replica without a map
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&samples[g], 1ull);
    const int ncap = tp.n_cap_atoms;
    const int i = blockIdx.x * kDensityBlock + threadIdx.x;
    int c = kDensityNone;
    if (i < ncap) {
        c = (int)(da.table >> (4 * tp.slot_ty[i])) & kDensityNone;
        if (c != kDensityNone && atom_mol[i] >= nmol[(size_t)replica * tp.n_res + atom_res[i]]) c = kDensityNone;   // unoccupied
    }
    if (__ballot(c != kDensityNone) == 0) return;                       // (per wave) none of these 64 slots has a channel
    if (c == kDensityNone) return;
    const double *px = pos + (size_t)replica * 3 * ncap;
    const double dx = px[i] - bx.lo[0], dy = px[ncap + i] - bx.lo[1], dz = px[2 * (size_t)ncap + i] - bx.lo[2];
    double s0, s1, s2;
    if (TRI) {
        s0 = bx.rcp[0] * dx + bx.rcp[1] * dy + bx.rcp[2] * dz;
        s1 = bx.rcp[3] * dx + bx.rcp[4] * dy + bx.rcp[5] * dz;
        s2 = bx.rcp[6] * dx + bx.rcp[7] * dy + bx.rcp[8] * dz;
    } else {
        s0 = dx * bx.invL[0]; s1 = dy * bx.invL[1]; s2 = dz * bx.invL[2];
    }
    const int v0 = density_voxel(s0, da.n[0]), v1 = density_voxel(s1, da.n[1]), v2 = density_voxel(s2, da.n[2]);
    const size_t map = (size_t)g * da.n_channels + c;
    atomicAdd(&hist[((map * da.n[2] + v2) * da.n[1] + v1) * da.n[0] + v0], 1ull);
}

}  // namespace mgpu

#endif
