// Per-molecule removal energies of MANY replicas per pass (mgpu_molecule_energies_replicas, mgpu_molecule_energy_*): for every
// molecule m of a selected ACTIVE residue type t, u[c](t, m) = E[c](X) - E[c](X without m) for the five components of
// ComputeSystemEnergy, computed from scratch in the static total's arithmetic.
//
//   real space   molen_sweep_kernel: epairs_sweep_kernel's frame -- work unit = (item, split), ONE WAVE each, persistent waves,
//                the Coulomb table and the pair table staged in LDS once per workgroup, the item's sites through the wave's LDS
//                slab kSiteChunk at a time, the three layouts of Topo::site_major -- with ONE difference: an item is molecule
//                (t, m) against ALL molecules of partner type t2, only m itself left out where t2 == t (m2 != m, not m2 > m).
//                Every pair is so evaluated once for each of its two molecules: scattering one evaluation to both would need
//                floating-point adds in launch order.  Every term is pair_term<true, TRI>.  (A kernel of its own, not a
//                predicate in epairs_sweep_kernel: that kernel's text and assembly stay as they are.)
//   reciprocal   the pass's phase tables and S(k) (phase_table_replicas_kernel, sfactor_replicas_kernel, unchanged), then
//                molen_recip_kernel, one workgroup per molecule: prefactor * sum_k ff W (2 Re(conj(S) A_m) - |A_m|^2) with
//                A_m(k) the molecule's own sum over its site slots from the same tables.  A(k) is neither read nor written.
//   reduction    molen_reduce_kernel, one thread per molecule: the partner types' results added in type order, the five
//                components and the total as serial chains of rounded adds; the row of `out`, or ONE integer add to the
//                replica's histogram.
// No floating-point atomics anywhere: every number is a function of the replica's configuration and of (t, m) alone.
#ifndef MGPU_KERNELS_MOLEN_H
#define MGPU_KERNELS_MOLEN_H

#include "mgpu_kernels_common.h"
#include "mgpu_kernels_epairs.h"

namespace mgpu {

constexpr int kMolenMaxBins = 4096;
// LDS of molen_recip_kernel's site tile: ktot table rows of as many sites as fit.  16 KiB keeps ten workgroups on a CU, holds a
// small molecule whole at any k table the engine admits, and makes a 64-site molecule loop over tiles from ktot = 17 on
constexpr size_t kMolenTileBytes = 16 * 1024;

// one molecule of a pass.  Its real-space items are EpItem [index * n_res + t2], t2 in type order; its intra item, its
// reciprocal result and this record share the index.
struct MolRec {
    int entry;                    // index of the replica within the pass (block of the phase tables and of S)
    int replica;
    int t, m;
    int sel;                      // index of t in the selection
    int row;                      // row of the replica's block of `out`
    int charged;                  // t has a charged site (else coulomb, recip, self and intra are exactly 0)
    int tile;                     // sites of t whose phase-table entries molen_recip_kernel stages in LDS at a time (0: none fit)
    double self_v;                // ComputeEwaldSelfInteractionSingleMol of t
};

// the histogram of the accumulate call: slot 0 below e_min, 1 .. n_bins inside, n_bins + 1 from e_max on (and not-a-number)
struct MolenBins {
    int n_bins, n_sel;
    double e_min, e_max, inv_w;   // inv_w = n_bins / (e_max - e_min), formed on the host
};

__device__ __forceinline__ int molen_slot(const MolenBins &b, double u) {
#pragma clang fp contract(off)
    if (u < b.e_min) return 0;
    if (u < b.e_max) {
        const double d = u - b.e_min;
        const double x = d * b.inv_w;
        return 1 + min(b.n_bins - 1, (int)floor(x));
    }
    return b.n_bins + 1;
}

template <bool TRI>
__global__ __launch_bounds__(kPairBlock, MGPU_PAIR_MINWAVES) void molen_sweep_kernel(
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
        // (uniform) nothing to sweep: the partner type is empty, or the item is the only molecule of its own type
        const bool any = nm > 0 && !(same_t && nm == 1);
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
                    if (same_t) valid = valid && m2 != it.m;
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
                    if (same_t && m2 == it.m) continue;
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

// ComputeReciprocalEnergy's prefactor times sum_k ff W (2 Re(conj(S) A_m) - |A_m|^2) for molecule blockIdx.x of the pass: S =
// block `entry` of the pass's structure factors (slot kslot[k]), A_m(k) = sum over the molecule's sites, in site order, of
// q exp(i k r) from table `entry` of the pass's phase tables, with sfactor_replicas_kernel's products.  Thread j takes k = j,
// j + kBlock, ... in ascending order, then wave_sum, the waves in order.  The table entries of `tile` sites at a time are staged
// in LDS ([row][site of the tile], ktot rows); a molecule of more sites than fit loops over site tiles, staged again for every
// kBlock k-vectors (the barriers are uniform: every thread walks every tile); tile = 0 reads the table in place.  A_m adds the
// sites in the same order whatever the tile.  A type without a charged site: exactly 0.
static __global__ __launch_bounds__(kBlock) void molen_recip_kernel(Topo tp, BoxDev bx, const double *__restrict__ kw,
                                                                    const int *__restrict__ kpack, const int *__restrict__ kslot,
                                                                    const double *__restrict__ atom_q,
                                                                    const MolRec *__restrict__ recs, size_t tab_stride,
                                                                    const double2 *__restrict__ tab_all,
                                                                    const double2 *__restrict__ S_all, double *__restrict__ u) {
    extern __shared__ __attribute__((aligned(16))) double2 s_tab[];     // [ktot][tile]
    __shared__ double s_red[kWavesPerBlock];
    const MolRec rc = recs[blockIdx.x];
    if (!rc.charged) {                                                  // (uniform)
        if (threadIdx.x == 0) u[blockIdx.x] = 0.0;
        return;
    }
    const double2 *tab = tab_all + (size_t)rc.entry * tab_stride;
    const double2 *S = S_all + (size_t)rc.entry * bx.n_slots;
    const size_t nc = tp.n_cap_atoms;
    const int n1 = tp.n1[rc.t];
    const int ktot = bx.kmax[0] + bx.kmax[1] + bx.kmax[2] + 3;
    const int row_y = bx.kmax[0] + 1, row_z = bx.kmax[0] + bx.kmax[1] + 2;
    const int tile = rc.tile;
    const int step = tile > 0 ? tile : n1;
    const bool one_tile = step >= n1;
    double acc = 0.0;
    for (int k0 = 0; k0 < bx.nk; k0 += kBlock) {
        const int k = k0 + threadIdx.x;
        const bool live = k < bx.nk;
        int kx = 0, ky = 0, kz = 0;
        if (live) {
            const int kp = kpack[k];
            kx = kp & 0xff; ky = ((kp >> 8) & 0xff) - 128; kz = ((kp >> 16) & 0xff) - 128;
        }
        const int aky = ky < 0 ? -ky : ky, akz = kz < 0 ? -kz : kz;
        double are = 0.0, aim = 0.0;
        for (int s0 = 0; s0 < n1; s0 += step) {
            const int ns = min(step, n1 - s0);
            if (tile > 0 && (k0 == 0 || !one_tile)) {
                __syncthreads();                                        // the previous tile has been read
                for (int i = threadIdx.x; i < ktot * ns; i += kBlock) {
                    const int row = i / ns, s = i - row * ns;
                    s_tab[row * tile + s] = tab[(size_t)row * nc + atom_slot(tp, rc.t, rc.m, s0 + s)];
                }
                __syncthreads();
            }
            if (live)
                for (int s = 0; s < ns; ++s) {
                    const int j = atom_slot(tp, rc.t, rc.m, s0 + s);
                    double2 X, Y, Z;
                    if (tile > 0) {
                        X = s_tab[kx * tile + s]; Y = s_tab[(row_y + aky) * tile + s]; Z = s_tab[(row_z + akz) * tile + s];
                    } else {
                        X = tab[(size_t)kx * nc + j]; Y = tab[(size_t)(row_y + aky) * nc + j]; Z = tab[(size_t)(row_z + akz) * nc + j];
                    }
                    if (ky < 0) Y.y = -Y.y;
                    if (kz < 0) Z.y = -Z.y;
                    const double2 p = cmul(cmul(X, Y), Z);
                    const double q = atom_q[j];
                    are += q * p.x;
                    aim += q * p.y;
                }
        }
        if (live) {
            const double2 s = S[kslot[k]];
            const double cross = fma(s.x, are, s.y * aim), own = fma(are, are, aim * aim);
            acc += kw[k] * (2.0 * cross - own);
        }
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

// The row of every molecule of a pass, one thread each: the partner types' LJ / Coulomb results added in type order, the five
// components and total = ((((nc + c) + r) + s) + i), every sum a serial chain of rounded adds.  out != null: the row
// out[entry][row][0..4] (the blocks of `out` are rows_per doubles x 5 apart).  hist != null: one add to slot
// hist[replica][sel][molen_slot(total)].  Threads n_mol .. n_mol + n_rep - 1 add the sample of the pass's replicas.
static __global__ __launch_bounds__(64) void molen_reduce_kernel(int n_res, const MolRec *__restrict__ recs, int n_mol,
                                                                 const int *__restrict__ reps, int n_rep,
                                                                 const double *__restrict__ lj, const double *__restrict__ coul,
                                                                 const double *__restrict__ intra,
                                                                 const double *__restrict__ u_recip, size_t rows_per,
                                                                 double *__restrict__ out, MolenBins bins,
                                                                 unsigned long long *__restrict__ hist,
                                                                 unsigned long long *__restrict__ samples) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mol) {
        if (hist && i < n_mol + n_rep) atomicAdd(samples + reps[i - n_mol], 1ull);
        return;
    }
    const MolRec &r = recs[i];
    double e_nc = 0.0, e_c = 0.0;
    for (int t2 = 0; t2 < n_res; ++t2) {
        e_nc = e_nc + lj[(size_t)i * n_res + t2];
        e_c = e_c + coul[(size_t)i * n_res + t2];
    }
    double e_r = 0.0, e_s = 0.0, e_i = 0.0;
    if (r.charged) { e_r = u_recip[i]; e_s = r.self_v; e_i = intra[i]; }
    if (out) {
        double *o = out + ((size_t)r.entry * rows_per + r.row) * 5;
        o[0] = e_nc; o[1] = e_c; o[2] = e_r; o[3] = e_s; o[4] = e_i;
    }
    if (hist) {
        const double total = ((((e_nc + e_c) + e_r) + e_s) + e_i);
        const size_t per = (size_t)bins.n_sel * (bins.n_bins + 2);
        atomicAdd(hist + (size_t)r.replica * per + (size_t)r.sel * (bins.n_bins + 2) + molen_slot(bins, total), 1ull);
    }
}

}  // namespace mgpu

#endif
