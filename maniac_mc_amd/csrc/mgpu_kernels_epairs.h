// Energies by residue-type pair of MANY replicas per pass (mgpu_energy_pairs_replicas): for every selected unordered pair
// (a, b) of residue types the five components of ComputeSystemEnergy restricted to that pair.  The pair-wise components are
// quadratic forms of the configuration, so the entries of the full matrix add back to the whole-system total.
//
//   real space   epairs_sweep_kernel: work unit = (item, split), ONE WAVE each, persistent waves, the Coulomb table and the pair
//                table staged in LDS once per workgroup.  An item is one molecule (t, m) against ONE partner type t2; its sites
//                pass through the wave's LDS slab kSiteChunk at a time (molecules of any size), the wave sweeps the occupied
//                slots of t2's segment -- only the molecules after m where t2 == t -- in the three layouts of Topo::site_major
//                and writes one partial {e_lj, e_coul}.  Every term is pair_term<true, TRI>: the arithmetic of the static
//                total's generic path.  A type that is not a partner of the item costs nothing.
//   reciprocal   sfactor_types_replicas_kernel on the grid (k, replica): the partial structure factors S_t(k) of the residue
//                types the selection names, each over its own slot segment with sfactor_replicas_kernel's thread stride and
//                reduction order, from the pass's phase tables (phase_table_replicas_kernel); then epairs_recip_kernel, one
//                workgroup per (replica, pair): prefactor * sum_k ff W F_ab, F_aa = |S_a|^2, F_ab = 2 Re(S_a conj S_b).
//                A(k) is neither read nor written.
//   reduction    epairs_reduce_kernel, one thread per (replica, pair): the items' results, then the intra results, added in
//                molecule order as serial chains of rounded adds; the self term as energy_reduce_replicas_kernel forms it.
// No floating-point atomics anywhere: every number is a function of the replica's configuration and of (a, b) alone, whatever
// shares the launch.
#ifndef MGPU_KERNELS_EPAIRS_H
#define MGPU_KERNELS_EPAIRS_H

#include "mgpu_kernels_common.h"
#include "mgpu_kernels_recip.h"

namespace mgpu {

constexpr int kEpairsMaxSel = 36;     // unordered pairs of kMaxRes residue types

// one molecule (t, m) of a replica against the molecules of type t2 (t2 == t: those after m only, each pair once)
struct EpItem { int replica, t, m, t2; };

// one (replica of the pass, selected pair): where its results lie in the pass's lists
struct EpRec {
    int entry;                    // index of the replica within the pass (block of the S_t scratch)
    int item_first, n_items;      // its real-space items (molecule order)
    int intra_first, n_intra;     // its intra items (a == b, ACTIVE type), else none
    int n_self;                   // molecules of type a where a == b, else 0
    int sa, sb;                   // index of a / b among the types whose S_t(k) the pass forms; < 0: no charged site
    int same;                     // a == b
    double self_v;                // ComputeEwaldSelfInteractionSingleMol of type a where a == b, else 0
};

struct EpTypes { int n; int t[kMaxRes]; };     // the residue types whose S_t(k) a pass forms

template <bool TRI>
__global__ __launch_bounds__(kPairBlock, MGPU_PAIR_MINWAVES) void epairs_sweep_kernel(
    Topo tp, BoxDev bx, const double *__restrict__ pos, const int *__restrict__ nmol, const double *__restrict__ res_q,
    const int *__restrict__ res_atype, const double2 *__restrict__ pair_tab, const char *__restrict__ coul_tab_g,
    const EpItem *__restrict__ items, int nsplit, int n_work, double2 *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) char s_coul[];     // (coul_last_row + 1) x 48 B
    __shared__ double2 s_pair[kMaxTypes * kMaxTypes];
    __shared__ double s_site[kPairWaves * kSiteChunk * 4];
    __shared__ int s_sty[kPairWaves * kSiteChunk];

    for (int i = threadIdx.x; i < (bx.coul_last_row + 1) * kCoulRowVec; i += kPairBlock)
        reinterpret_cast<double2 *>(s_coul)[i] = reinterpret_cast<const double2 *>(coul_tab_g)[i];
    const int nt = tp.n_types;
    for (int i = threadIdx.x; i < nt * nt; i += kPairBlock) s_pair[i] = pair_tab[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = gridDim.x * kPairWaves;
    double *w_site = s_site + wave * kSiteChunk * 4;
    int *w_sty = s_sty + wave * kSiteChunk;

    for (int w = blockIdx.x * kPairWaves + wave; w < n_work; w += n_waves) {
        const int item_id = w / nsplit, split = w - item_id * nsplit;
        const EpItem it = items[item_id];
        const double *px = pos + (size_t)it.replica * 3 * tp.n_cap_atoms;
        const double *py = px + tp.n_cap_atoms, *pz = py + tp.n_cap_atoms;
        const int t2 = it.t2;
        const int n1 = tp.n1[it.t], n2 = tp.n1[t2];
        const int nm = nmol[it.replica * tp.n_res + t2];
        const bool same_t = t2 == it.t;
        const int seg2 = tp.seg_off[t2], cap2 = tp.cap[t2];
        double elj = 0.0, ec = 0.0;
        // (uniform) nothing to sweep: the partner type is empty, or no molecule of the item's own type lies after it
        const bool any = nm > 0 && !(same_t && it.m + 1 >= nm);
        for (int sb = 0; any && sb < n1; sb += kSiteChunk) {
            const int ns = min(kSiteChunk, n1 - sb);
            // this chunk of the item's sites into the wave's own LDS slab (no workgroup barrier needed)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane < ns) {
                const int j = atom_slot(tp, it.t, it.m, sb + lane);
                w_site[lane * 4 + 0] = px[j]; w_site[lane * 4 + 1] = py[j]; w_site[lane * 4 + 2] = pz[j];
                w_site[lane * 4 + 3] = res_q[it.t * tp.max_atom + sb + lane];
                w_sty[lane] = res_atype[it.t * tp.max_atom + sb + lane];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (!tp.site_major[t2]) {
                // plane-major: unit = (site index a2, 64 consecutive molecules); q / type uniform
                const int cpp = (nm + 63) >> 6, units = n2 * cpp;
                for (int u = split; u < units; u += nsplit) {
                    const int a2 = u / cpp, m2 = (u - a2 * cpp) * 64 + lane;
                    bool valid = m2 < nm;
                    if (same_t) valid = valid && m2 > it.m;
                    const double qj = res_q[t2 * tp.max_atom + a2];
                    const int tyj = res_atype[t2 * tp.max_atom + a2];
                    const bool qj_on = fabs(qj) >= kErrorTol;
                    double xj = 0.0, yj = 0.0, zj = 0.0;
                    if (valid) {
                        const int j = seg2 + a2 * cap2 + m2;
                        xj = px[j]; yj = py[j]; zj = pz[j];
                    }
                    for (int s = 0; s < ns; ++s) {
                        const double qs = w_site[s * 4 + 3];
                        const double2 pt = s_pair[w_sty[s] * nt + tyj];
                        const bool do_c = qj_on && (fabs(qs) >= kErrorTol);   // energy_utils.f90:430
                        const bool do_lj = pt.x != 0.0;                        // epsilon = 0 contributes 0
                        if ((do_c || do_lj) && valid)
                            pair_term<true, TRI>(xj - w_site[s * 4 + 0], yj - w_site[s * 4 + 1], zj - w_site[s * 4 + 2], bx, qs * qj,
                                                 pt.x, pt.y, do_lj, do_c, s_coul, elj, ec);
                    }
                }
            } else {
                // site-major and frozen: unit = (molecule m2, 64 consecutive sites); per-lane q / type (a frozen type's
                // templates are held in its sorted site order, as its slots are)
                const int cpp = (n2 + 63) >> 6, units = nm * cpp;
                for (int u = split; u < units; u += nsplit) {
                    const int m2 = u / cpp, a2 = (u - m2 * cpp) * 64 + lane;
                    if (same_t && m2 <= it.m) continue;
                    const bool valid = a2 < n2;
                    double xj = 0.0, yj = 0.0, zj = 0.0, qj = 0.0;
                    int tyj = 0;
                    if (valid) {
                        const int j = seg2 + m2 * n2 + a2;
                        xj = px[j]; yj = py[j]; zj = pz[j];
                        qj = res_q[t2 * tp.max_atom + a2];
                        tyj = res_atype[t2 * tp.max_atom + a2];
                    }
                    const bool qj_on = fabs(qj) >= kErrorTol;
                    for (int s = 0; s < ns; ++s) {
                        const double qs = w_site[s * 4 + 3];
                        const double2 pt = s_pair[w_sty[s] * nt + tyj];
                        const bool do_c = qj_on && (fabs(qs) >= kErrorTol);
                        const bool do_lj = pt.x != 0.0;
                        if (valid && (do_lj || do_c))
                            pair_term<true, TRI>(xj - w_site[s * 4 + 0], yj - w_site[s * 4 + 1], zj - w_site[s * 4 + 2], bx, qs * qj,
                                                 pt.x, pt.y, do_lj, do_c, s_coul, elj, ec);
                    }
                }
            }
        }
        const double a = wave_sum(elj), b = wave_sum(ec);
        if (lane == 0) partials[w] = make_double2(a, b);
    }
}

// S_t(k) of the residue types ty.t[0 .. ty.n) for the replicas reps[blockIdx.y], from table blockIdx.y of `tab_all`: every
// (replica, type, k) sum adds the occupied atoms of the type's own slot segment as sfactor_replicas_kernel adds a replica's --
// thread stride kBlock from the segment's first slot, wave_sum, the waves in order.  S_all [pass entry][type][nk], k in the
// reference's order.
static __global__ __launch_bounds__(kBlock) void sfactor_types_replicas_kernel(Topo tp, BoxDev bx, const int *__restrict__ nmol,
                                                                               const int *__restrict__ atom_mol,
                                                                               const double *__restrict__ atom_q,
                                                                               const int *__restrict__ kpack,
                                                                               const int *__restrict__ reps, size_t tab_stride,
                                                                               const double2 *__restrict__ tab_all, EpTypes ty,
                                                                               double2 *__restrict__ S_all) {
    __shared__ double s_red[2 * kWavesPerBlock];
    const int k = blockIdx.x;
    const int replica = reps[blockIdx.y];
    const double2 *tab = tab_all + (size_t)blockIdx.y * tab_stride;
    const int kp = kpack[k];
    const int kx = kp & 0xff, ky = ((kp >> 8) & 0xff) - 128, kz = ((kp >> 16) & 0xff) - 128;
    const int aky = ky < 0 ? -ky : ky, akz = kz < 0 ? -kz : kz;
    const size_t nc = tp.n_cap_atoms;
    const double2 *tx = tab + (size_t)kx * nc;
    const double2 *ty_ = tab + (size_t)(bx.kmax[0] + 1 + aky) * nc;
    const double2 *tz = tab + (size_t)(bx.kmax[0] + bx.kmax[1] + 2 + akz) * nc;
    for (int i = 0; i < ty.n; ++i) {
        const int t = ty.t[i];
        const int nm = nmol[replica * tp.n_res + t];
        const int j0 = tp.seg_off[t], j1 = j0 + tp.n1[t] * tp.cap[t];
        double re = 0.0, im = 0.0;
        for (int j = j0 + threadIdx.x; nm > 0 && j < j1; j += kBlock) {
            if (atom_mol[j] >= nm) continue;
            double2 Y = ty_[j], Z = tz[j];
            if (ky < 0) Y.y = -Y.y;
            if (kz < 0) Z.y = -Z.y;
            const double2 p = cmul(cmul(tx[j], Y), Z);
            const double q = atom_q[j];
            re += q * p.x;
            im += q * p.y;
        }
        re = wave_sum(re);
        im = wave_sum(im);
        __syncthreads();                                            // the previous type's sums have been read
        if ((threadIdx.x & 63) == 0) { s_red[2 * (threadIdx.x >> 6)] = re; s_red[2 * (threadIdx.x >> 6) + 1] = im; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0, b = 0.0;
            for (int w = 0; w < kWavesPerBlock; ++w) { a += s_red[2 * w]; b += s_red[2 * w + 1]; }
            S_all[((size_t)blockIdx.y * ty.n + i) * bx.nk + k] = make_double2(a, b);
        }
    }
}

// ComputeReciprocalEnergy's prefactor times sum_k ff W F_ab for record blockIdx.x: thread j takes k = j, j + kBlock, ... in
// ascending order, wave_sum, the waves in order.  A pair with a type without a charged site: exactly 0.
static __global__ __launch_bounds__(kBlock) void epairs_recip_kernel(BoxDev bx, const double *__restrict__ kw,
                                                                     const EpRec *__restrict__ recs, int n_types,
                                                                     const double2 *__restrict__ S_all, double *__restrict__ u) {
    __shared__ double s_red[kWavesPerBlock];
    const EpRec &rc = recs[blockIdx.x];
    const int sa = rc.sa, sb = rc.sb;
    if (sa < 0 || sb < 0) {                                             // (uniform)
        if (threadIdx.x == 0) u[blockIdx.x] = 0.0;
        return;
    }
    const double2 *Sa = S_all + ((size_t)rc.entry * n_types + sa) * bx.nk;
    const double2 *Sb = S_all + ((size_t)rc.entry * n_types + sb) * bx.nk;
    const bool same = rc.same != 0;
    double acc = 0.0;
    for (int k = threadIdx.x; k < bx.nk; k += kBlock) {
        const double2 a = Sa[k];
        double f;
        if (same) {
            f = fma(a.x, a.x, a.y * a.y);
        } else {
            const double2 b = Sb[k];
            f = 2.0 * fma(a.x, b.x, a.y * b.y);
        }
        acc += kw[k] * f;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) s += s_red[w];
        u[blockIdx.x] = s * kEps0InvEvA / kKbEvK * kTwoPi / bx.volume;   // ewald_energy.f90:272
    }
}

// The five numbers of every (replica, pair) of a pass, one thread each: the items' LJ / Coulomb results and the intra results
// added in molecule order, every running sum a serial chain of rounded adds; the self term as energy_reduce_replicas_kernel
// forms one type's.  out[record][5].
static __global__ __launch_bounds__(64) void epairs_reduce_kernel(const EpRec *__restrict__ recs, int n, const double *__restrict__ lj,
                                                                  const double *__restrict__ coul, const double *__restrict__ intra,
                                                                  const double *__restrict__ u_recip, double *__restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const EpRec &r = recs[i];
    double e_nc = 0.0, e_c = 0.0, e_intra = 0.0;
    for (int k = 0; k < r.n_items; ++k) {
        e_nc = e_nc + lj[r.item_first + k];
        e_c = e_c + coul[r.item_first + k];
    }
    for (int k = 0; k < r.n_intra; ++k) e_intra = e_intra + intra[r.intra_first + k];
    double e_self = 0.0;
    if (r.same) {
        double s = r.self_v;
        s = s * (double)r.n_self;
        e_self = e_self + s;
    }
    double *o = out + (size_t)i * 5;
    o[0] = e_nc; o[1] = e_c; o[2] = u_recip[i]; o[3] = e_self; o[4] = e_intra;
}

}  // namespace mgpu

#endif
