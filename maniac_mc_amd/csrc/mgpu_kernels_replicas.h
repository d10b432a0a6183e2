// Whole-system energies and S(k) of MANY replicas per pass (mgpu_system_energy_replicas, mgpu_init_structure_factor_replicas):
// the batched forms of phase_table_kernel / sfactor_kernel, the ordered reduction of the per-molecule results and the
// deviation max |A - S|.  Everything here repeats, per replica, the arithmetic of the per-replica path in its order: the
// results are the per-replica calls' bit for bit, whatever shares the launch.
#ifndef MGPU_KERNELS_REPLICAS_H
#define MGPU_KERNELS_REPLICAS_H

#include "mgpu_kernels_common.h"
#include "mgpu_kernels_recip.h"

namespace mgpu {

// one replica of a pass: where its items lie in the pass's item lists, and its molecule counts
struct EnergyRep {
    int replica;
    int pair_first;               // first ordered pair item (its lj / coulomb results): one per molecule, (type, molecule) order
    int intra_first;              // first intra item: the ACTIVE types' molecules in the same order
    int n[kMaxRes];
};
struct SelfTerms { double v[kMaxRes]; };   // ComputeEwaldSelfInteractionSingleMol per residue type

// phase_table_kernel for the replicas reps[blockIdx.y]: table blockIdx.y of `tab`, tab_stride entries each
static __global__ void phase_table_replicas_kernel(Topo tp, BoxDev bx, const double *__restrict__ pos, const int *__restrict__ nmol,
                                                   const int *__restrict__ atom_res, const int *__restrict__ atom_mol,
                                                   const int *__restrict__ reps, size_t tab_stride, double2 *__restrict__ tab_all) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= tp.n_cap_atoms) return;
    const int replica = reps[blockIdx.y];
    double2 *tab = tab_all + (size_t)blockIdx.y * tab_stride;
    const int t = atom_res[j];
    if (atom_mol[j] >= nmol[replica * tp.n_res + t]) return;
    const double *px = pos + (size_t)replica * 3 * tp.n_cap_atoms;
    const double x = px[j], y = px[tp.n_cap_atoms + j], z = px[2 * tp.n_cap_atoms + j];
    int row = 0;
    for (int axis = 0; axis < 3; ++axis) {
        const double th = atom_phase(bx, axis, x, y, z);
        for (int k = 0; k <= bx.kmax[axis]; ++k, ++row) tab[(size_t)row * tp.n_cap_atoms + j] = phase_entry(th, k);
    }
}

// sfactor_kernel on the grid (k, replica of the pass): every (replica, k) sum adds its atoms as sfactor_kernel does -- thread
// j-stride of kBlock, wave_sum, the waves in order.  to_replica = 0: S(k) of pass entry i into block i of S (a scratch);
// 1: into block reps[i] (the replicas' A(k)).
static __global__ __launch_bounds__(kBlock) void sfactor_replicas_kernel(Topo tp, BoxDev bx, const int *__restrict__ nmol,
                                                                         const int *__restrict__ atom_res,
                                                                         const int *__restrict__ atom_mol,
                                                                         const double *__restrict__ atom_q,
                                                                         const int *__restrict__ kpack, const int *__restrict__ kslot,
                                                                         const int *__restrict__ reps, size_t tab_stride,
                                                                         const double2 *__restrict__ tab_all, int to_replica,
                                                                         double2 *__restrict__ S_all) {
    __shared__ double s_red[2 * kWavesPerBlock];
    const int k = blockIdx.x;
    const int replica = reps[blockIdx.y];
    const double2 *tab = tab_all + (size_t)blockIdx.y * tab_stride;
    double2 *S = S_all + (size_t)(to_replica ? replica : (int)blockIdx.y) * bx.n_slots;
    const int kp = kpack[k];
    const int kx = kp & 0xff, ky = ((kp >> 8) & 0xff) - 128, kz = ((kp >> 16) & 0xff) - 128;
    const int aky = ky < 0 ? -ky : ky, akz = kz < 0 ? -kz : kz;
    const size_t nc = tp.n_cap_atoms;
    const double2 *tx = tab + (size_t)kx * nc;
    const double2 *ty = tab + (size_t)(bx.kmax[0] + 1 + aky) * nc;
    const double2 *tz = tab + (size_t)(bx.kmax[0] + bx.kmax[1] + 2 + akz) * nc;
    double re = 0.0, im = 0.0;
    for (int j = threadIdx.x; j < tp.n_cap_atoms; j += kBlock) {
        if (atom_mol[j] >= nmol[replica * tp.n_res + atom_res[j]]) continue;
        double2 Y = ty[j], Z = tz[j];
        if (ky < 0) Y.y = -Y.y;
        if (kz < 0) Z.y = -Z.y;
        const double2 p = cmul(cmul(tx[j], Y), Z);
        const double q = atom_q[j];
        re += q * p.x;
        im += q * p.y;
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if ((threadIdx.x & 63) == 0) { s_red[2 * (threadIdx.x >> 6)] = re; s_red[2 * (threadIdx.x >> 6) + 1] = im; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) { a += s_red[2 * w]; b += s_red[2 * w + 1]; }
        S[kslot[k]] = make_double2(a, b);
    }
}

// ComputeSystemEnergy's sums for the replicas of a pass, one thread each: the per-molecule LJ / Coulomb results and the active
// types' intra results added in (type, molecule) order, every running sum a serial chain of rounded adds (mgpu_system_energy's
// host loop); the self term and the total as it forms them.  out[first + i][6].
// (the record is read in place: a private copy indexed by t would be promoted to LDS)
static __global__ __launch_bounds__(64) void energy_reduce_replicas_kernel(int n_res, const EnergyRep *__restrict__ reps, int n,
                                                                           unsigned active_mask, SelfTerms self,
                                                                           const double *__restrict__ lj, const double *__restrict__ coul,
                                                                           const double *__restrict__ intra,
                                                                           const double *__restrict__ u_recip, double *__restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const EnergyRep &r = reps[i];
    double e_nc = 0.0, e_c = 0.0, e_intra = 0.0;
    int at = r.pair_first, ii = r.intra_first;
    for (int t = 0; t < n_res; ++t)
        for (int m = 0; m < r.n[t]; ++m, ++at) {
            e_nc = e_nc + lj[at];
            e_c = e_c + coul[at];
            if ((active_mask >> t) & 1u) e_intra = e_intra + intra[ii++];
        }
    double e_self = 0.0;
    for (int t = 0; t < n_res; ++t) {
        double s = self.v[t];
        s = s * (double)r.n[t];
        e_self = e_self + s;
    }
    const double e_recip = u_recip[i];
    double *o = out + (size_t)i * 6;
    o[0] = e_nc; o[1] = e_c; o[2] = e_recip; o[3] = e_self; o[4] = e_intra;
    o[5] = e_recip + e_nc + e_c + e_self + e_intra;
}

// max over the k-vectors of max(|Re(A - S)|, |Im(A - S)|): A = A(k) of replica reps[i] (block reps[i] of A_all), S = block i of
// the pass's scratch.  One workgroup per replica; a maximum does not depend on the order it is taken in.
static __global__ __launch_bounds__(kBlock) void a_deviation_replicas_kernel(BoxDev bx, const int *__restrict__ kslot,
                                                                             const int *__restrict__ reps,
                                                                             const double2 *__restrict__ A_all,
                                                                             const double2 *__restrict__ S_all, double *__restrict__ dev) {
    __shared__ double s_red[kWavesPerBlock];
    const int i = blockIdx.x;
    const double2 *A = A_all + (size_t)reps[i] * bx.n_slots;
    const double2 *S = S_all + (size_t)i * bx.n_slots;
    double d = 0.0;
    for (int k = threadIdx.x; k < bx.nk; k += kBlock) {
        const int s = kslot[k];
        const double2 a = A[s], b = S[s];
        d = fmax(d, fmax(fabs(a.x - b.x), fabs(a.y - b.y)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d = fmax(d, __shfl_xor(d, off, 64));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w) d = fmax(d, s_red[w]);
        dev[i] = d;
    }
}

}  // namespace mgpu

#endif
