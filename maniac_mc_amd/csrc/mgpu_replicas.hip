// Whole-system energies and S(k) for many replicas per call: mgpu_system_energy_replicas and
// mgpu_init_structure_factor_replicas, the batched twins of mgpu_system_energy and mgpu_init_structure_factor
// (mgpu_engine.hip).  A call is cut into passes of as many replicas as a byte budget of scratch allows; a pass is one
// ordered pair launch, one intra launch, one phase-table + S(k) launch pair, one reciprocal-energy launch, one reduction
// (and one deviation launch) for all its replicas.  Nothing is waited for between the passes; one copy brings the results back.
// Beside them the radial distribution functions of many replicas per call (mgpu_rdf_*): integer histograms of the resident
// coordinates, one rdf_hist_kernel launch per pass.  And the energies by residue-type pair (mgpu_energy_pairs_replicas): passes of
// the same budget, per pass one sweep over (molecule, partner type) items, the partial structure factors of the selected types
// and one ordered reduction per (replica, pair).  And the density maps (mgpu_density_*): integer counts per voxel of selected
// atom types, pooled per group of replicas, one density_map_kernel launch per pass.  And the per-molecule removal energies
// (mgpu_molecule_energies_replicas, mgpu_molecule_energy_*): passes of the energy calls' budget, per pass one sweep over
// (molecule, partner type) items, the pass's S(k), one workgroup per molecule for its reciprocal part and one thread per molecule
// for its row or its histogram slot.
// What the analyses share has one home each: the passes of the two energy calls are plan_passes (mgpu_internal.h), every list
// of replicas or groups goes through check_index_list, the accumulators of rdf and density are an Accum (mgpu_internal.h) read,
// loaded and cleared by accum_read / accum_load / accum_reset, their packed type tables are built with nibble_get / nibble_set,
// and the phase tables of a pass are launched by launch_phase_tables_replicas.
#include "mgpu_engine.h"
#include "mgpu_kernels_replicas.h"
#include "mgpu_kernels_rdf.h"
#include "mgpu_kernels_density.h"
#include "mgpu_kernels_epairs.h"
#include "mgpu_kernels_molen.h"

namespace mgpu {

// a list of n distinct indices below `limit`: replicas, or the groups of the density maps (`noun`)
static int check_index_list(int n, const int *ids, int limit, const char *noun, const char *who) {
    if (n < 0 || (n > 0 && !ids)) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": bad " + noun + " list");
    std::vector<char> seen((size_t)limit, 0);
    for (int i = 0; i < n; ++i) {
        const int r = ids[i];
        if (r < 0 || r >= limit) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": " + noun + " out of range");
        if (seen[r]) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": " + noun + " " + std::to_string(r) + " listed twice");
        seen[r] = 1;
    }
    return MGPU_OK;
}

static size_t phase_tab_entries(const mgpu_engine *e) { return (size_t)recip_ktot(e) * e->tp.n_cap_atoms; }

// the phase tables of the replicas d_reps[0 .. c) into d_tab
static void launch_phase_tables_replicas(mgpu_engine *e, const int *d_reps, int c, double2 *d_tab) {
    hipLaunchKernelGGL(phase_table_replicas_kernel, dim3((e->tp.n_cap_atoms + 255) / 256, c), dim3(256), 0, e->stream, e->tp, e->bx,
                       e->d_pos, e->d_nmol, e->d_atom_res, e->d_atom_mol, d_reps, phase_tab_entries(e), d_tab);
}

// the phase tables of the replicas d_reps[0 .. c) into d_tab, then their S(k): into block i of S_all (to_replica = false) or
// into block d_reps[i] (true: S_all = the replicas' A(k))
static int launch_sfactor_replicas(mgpu_engine *e, const int *d_reps, int c, double2 *d_tab, bool to_replica, double2 *S_all) {
    hipEvent_t a = nullptr, b = nullptr;
    int rc = prof_begin(e, e->lanes[0], MGPU_KERNEL_SFACTOR, &a, &b);
    if (rc) return rc;
    launch_phase_tables_replicas(e, d_reps, c, d_tab);
    hipExtLaunchKernelGGL(sfactor_replicas_kernel, dim3(e->nk, c), dim3(kBlock), 0, e->stream, a, b, 0, e->tp, e->bx, e->d_nmol,
                          e->d_atom_res, e->d_atom_mol, e->d_atom_q, e->d_kpack, e->d_kslot, d_reps, phase_tab_entries(e),
                          (const double2 *)d_tab, to_replica ? 1 : 0, S_all);
    rc = prof_end(e, e->lanes[0], MGPU_KERNEL_SFACTOR, a, b);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// ---- the accumulators of rdf and density: segment s of the block, and the three calls on a checked list of entries.  `host[s]`
// holds the listed entries' words of segment s, entry after entry.
static unsigned long long *accum_seg(const Accum &a, const DevBuf &d_acc, int s) { return (unsigned long long *)d_acc.p + a.at[s]; }

// whole = true: one copy of the whole block and a scatter on the host (a farm checkpoint reads every replica: a few small
// copies per entry would be slower); false: one copy per entry and segment (a block may be large, and few entries wanted)
static int accum_read(const Accum &a, const DevBuf &d_acc, int n, const int *ids, unsigned long long *const host[3], bool whole) {
    std::vector<unsigned long long> all;
    if (whole) {
        all.resize(a.words);
        HIP_TRY(hipMemcpy(all.data(), d_acc.p, a.bytes(), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < a.n_seg; ++s) {
            const size_t at = a.word(s, (size_t)ids[i]), bytes = a.per[s] * sizeof(unsigned long long);
            if (whole) std::memcpy(host[s] + (size_t)i * a.per[s], all.data() + at, bytes);
            else HIP_TRY(hipMemcpy(host[s] + (size_t)i * a.per[s], (const unsigned long long *)d_acc.p + at, bytes, hipMemcpyDeviceToHost));
        }
    return MGPU_OK;
}

static int accum_load(const Accum &a, const DevBuf &d_acc, int n, const int *ids, const unsigned long long *const host[3]) {
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < a.n_seg; ++s)
            HIP_TRY(hipMemcpy((unsigned long long *)d_acc.p + a.word(s, (size_t)ids[i]), host[s] + (size_t)i * a.per[s],
                              a.per[s] * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return MGPU_OK;
}

static int accum_reset(const Accum &a, const DevBuf &d_acc, int n, const int *ids) {
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < a.n_seg; ++s)
            HIP_TRY(hipMemset((unsigned long long *)d_acc.p + a.word(s, (size_t)ids[i]), 0, a.per[s] * sizeof(unsigned long long)));
    return MGPU_OK;
}

// ---- radial distribution functions
static_assert(kRdfNone == (int)kNibbleNone && kDensityNone == (int)kNibbleNone, "the kernels read the tables nibble_set packs");

// half the smallest perpendicular width of the cell: the largest r_max a histogram may have.  Orthorhombic: min L / 2;
// triclinic: width i = V / |a_j x a_k| from box%matrix (its columns are the cell vectors).  Plain rounded operations in a
// fixed order (maniac_mc_amd/rdf.py half_width forms the same double).
static double rdf_half_width(const mgpu_engine *e) {
#pragma clang fp contract(off)
    const double *m = e->box_matrix;
    if (!e->bx.triclinic) return 0.5 * std::min(m[0], std::min(m[4], m[8]));
    double v[3][3];
    for (int k = 0; k < 3; ++k) { v[k][0] = m[k]; v[k][1] = m[3 + k]; v[k][2] = m[6 + k]; }
    auto cross = [](const double *a, const double *b, double *c) {
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
    };
    double bc[3];
    cross(v[1], v[2], bc);
    const double vol = std::fabs(v[0][0] * bc[0] + v[0][1] * bc[1] + v[0][2] * bc[2]);
    double least = 0.0;
    for (int i = 0; i < 3; ++i) {
        double c[3];
        cross(v[(i + 1) % 3], v[(i + 2) % 3], c);
        const double w = vol / std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (i == 0 || w < least) least = w;
    }
    return 0.5 * least;
}

static std::string rdf_number(double v) {
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// the replica list of an mgpu_rdf_* call, then "configured": in this order
static int rdf_ready(const mgpu_engine *e, int n, const int *replicas, const char *who) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    const int rc = check_index_list(n, replicas, e->n_replicas, "replica", who);
    if (rc) return rc;
    if (e->rdf.n_pairs == 0) return set_error(MGPU_ERR_STATE, std::string(who) + ": no histogram is configured (mgpu_rdf_configure)");
    return MGPU_OK;
}

// ---- density maps
static int density_ready(const mgpu_engine *e, const char *who) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (e->density.n_channels == 0) return set_error(MGPU_ERR_STATE, std::string(who) + ": no density map is configured (mgpu_density_configure)");
    return MGPU_OK;
}

// "configured", then the group list of an mgpu_density_read / _load / _reset call: in this order
static int density_groups_ready(const mgpu_engine *e, int n, const int *groups, const char *who) {
    const int rc = density_ready(e, who);
    return rc ? rc : check_index_list(n, groups, e->density.n_groups, "group", who);
}

// ---- per-molecule removal energies
// the selection of an mgpu_molecule_energies_replicas / mgpu_molecule_energy_configure call: 1 to kMaxRes distinct ACTIVE types
static int molen_check_types(const mgpu_engine *e, int n_sel, const int *types, const char *who) {
    if (n_sel < 1 || n_sel > kMaxRes)
        return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": n_sel " + std::to_string(n_sel) + " types is outside [1, " +
                         std::to_string(kMaxRes) + "]");
    if (!types) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": null type list");
    bool taken[kMaxRes] = {};
    for (int s = 0; s < n_sel; ++s) {
        const int t = types[s];
        const std::string name = ": type " + std::to_string(s) + " (residue type " + std::to_string(t) + ")";
        if (t < 0 || t >= e->tp.n_res)
            return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + name + " is out of range [0, " + std::to_string(e->tp.n_res - 1) + "]");
        if (e->is_active[t] != 1) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + name + " is not an active type");
        if (taken[t]) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + name + " is a duplicate");
        taken[t] = true;
    }
    return MGPU_OK;
}

// The passes of both molecule-energy calls over a checked replica list and selection: the same kernels in the same order.
// out != null (the stateless call): every pass's rows [c][rows][5] come back behind it, and counts [n][n_sel] is filled from
// the host's molecule counts.  bins != null (the accumulate call): every molecule's total goes into the engine's histograms,
// nothing comes back.
static int molen_passes(mgpu_engine *e, int n, const int *replicas, int chunk, int n_sel, const int *types, double *out, int *counts,
                        const MolenBins *bins, const char *who) {
    int rc;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const Topo &tp = e->tp;
    const int n_res = tp.n_res, nsplit = e->pair_nsplit;
    const size_t tab_n = phase_tab_entries(e);
    const int ktot = recip_ktot(e);
    size_t rows = 0;
    int row_first[kMaxRes], tile_of[kMaxRes], charged_of[kMaxRes];
    double self_of[kMaxRes];
    bool any_charged = false;
    int max_tile = 0;
    for (int s = 0; s < n_sel; ++s) {
        const int t = types[s];
        row_first[s] = (int)rows;
        rows += (size_t)e->mol_capacity[t];
        bool charged = false;
        for (int a = 0; a < tp.n1[t]; ++a) charged = charged || std::fabs(e->charges[(size_t)t * tp.max_atom + a]) >= kErrorTol;
        charged_of[s] = charged ? 1 : 0;
        // the sites whose table entries fit the reciprocal kernel's LDS tile: fixed by the type and the k table alone
        tile_of[s] = std::min(tp.n1[t], (int)(kMolenTileBytes / ((size_t)ktot * kLdsPhase)));
        self_of[s] = self_energy_host(e, t);
        if (charged) { any_charged = true; max_tile = std::max(max_tile, tile_of[s]); }
    }
    const size_t recip_lds = (size_t)ktot * max_tile * kLdsPhase;
    const size_t row_bytes = out ? rows * 5 * sizeof(double) : 0;
    auto counts_of = [&](int i, long long &n_it, long long &n_mol) {
        n_mol = 0;
        for (int s = 0; s < n_sel; ++s) n_mol += e->h_nmol[replicas[i] * n_res + types[s]];
        n_it = n_mol * n_res;
    };
    const size_t s_n = any_charged ? tab_n + e->n_slots : 0;           // complex entries of a replica's tables and S(k)
    // what a replica adds to a pass: its tables and S(k), its items, their split partials and results, its records and rows
    auto bytes_of = [&](long long n_it, long long n_mol) {
        return s_n * sizeof(double2) + (size_t)n_it * sizeof(EpItem) + (size_t)n_mol * (sizeof(PairItem) + sizeof(MolRec)) +
               (size_t)n_it * nsplit * sizeof(double2) + (size_t)(2 * n_it + 2 * n_mol) * sizeof(double) + sizeof(int) + row_bytes;
    };
    std::vector<Pass> passes;
    if (!plan_passes(n, counts_of, bytes_of, chunk, nsplit, passes))
        return set_error(MGPU_ERR_CAPACITY, std::string(who) + ": one replica's sweep exceeds 2^31 work units");
    size_t max_tab = 0, max_items = 0, max_rec = 0, max_res = 0, max_part = 0;
    for (const Pass &p : passes) {
        max_tab = std::max(max_tab, (size_t)p.c * s_n * sizeof(double2));
        max_items = std::max(max_items, (size_t)p.n_pair * sizeof(EpItem) + (size_t)p.n_in * sizeof(PairItem));
        max_rec = std::max(max_rec, (size_t)p.n_in * sizeof(MolRec) + (size_t)p.c * sizeof(int));
        max_res = std::max(max_res, (size_t)p.c * row_bytes + (size_t)(2 * p.n_pair + 2 * p.n_in) * sizeof(double));
        max_part = std::max(max_part, (size_t)p.n_pair * nsplit * sizeof(double2));
    }
    // every block is reserved once, before the first pass: nothing is freed under a pass still in flight
    if ((rc = e->d_out.reserve(std::max<size_t>(max_res, 8)))) return rc;
    if ((rc = e->d_items.reserve(std::max<size_t>(max_items, 8)))) return rc;
    if ((rc = e->d_items2.reserve(std::max<size_t>(max_rec, 8)))) return rc;
    if ((rc = e->d_partials.reserve(std::max<size_t>(max_part, 16)))) return rc;
    if ((rc = e->lanes[0].d_scratch.reserve(std::max<size_t>(max_tab, 16)))) return rc;
    const MolenBins no_bins{};
    // the host images of the passes' uploads live until the stream has been waited for
    std::deque<std::vector<char>> h_items, h_recs;
    for (const Pass &p : passes) {
        const int c = p.c, n_it = (int)p.n_pair, n_mol = (int)p.n_in;
        h_items.emplace_back((size_t)n_it * sizeof(EpItem) + (size_t)n_mol * sizeof(PairItem));
        EpItem *items = (EpItem *)h_items.back().data();
        PairItem *in_items = (PairItem *)(h_items.back().data() + (size_t)n_it * sizeof(EpItem));
        h_recs.emplace_back((size_t)n_mol * sizeof(MolRec) + (size_t)c * sizeof(int));
        MolRec *recs = (MolRec *)h_recs.back().data();
        int *idx = (int *)(h_recs.back().data() + (size_t)n_mol * sizeof(MolRec));
        int at = 0;
        for (int i = 0; i < c; ++i) {
            const int r = replicas[p.first + i];
            idx[i] = r;
            for (int s = 0; s < n_sel; ++s) {
                const int t = types[s], nm = e->h_nmol[r * n_res + t];
                if (counts) counts[(size_t)(p.first + i) * n_sel + s] = nm;
                for (int m = 0; m < nm; ++m, ++at) {
                    recs[at] = MolRec{i, r, t, m, s, row_first[s] + m, charged_of[s], tile_of[s], self_of[s]};
                    for (int t2 = 0; t2 < n_res; ++t2) items[(size_t)at * n_res + t2] = EpItem{r, t, m, t2};
                    in_items[at] = PairItem{r, t, m, -1, 0};
                }
            }
        }
        HIP_TRY(hipMemcpyAsync(e->d_items2.p, h_recs.back().data(), h_recs.back().size(), hipMemcpyHostToDevice, e->stream));
        const MolRec *d_recs = (const MolRec *)e->d_items2.p;
        const int *d_idx = (const int *)((const char *)e->d_items2.p + (size_t)n_mol * sizeof(MolRec));
        double *d_rows = (double *)e->d_out.p, *d_lj = (double *)((char *)e->d_out.p + (size_t)c * row_bytes);
        double *d_c = d_lj + n_it, *d_in = d_c + n_it, *d_u = d_in + n_mol;
        if (out) HIP_TRY(hipMemsetAsync(d_rows, 0, (size_t)c * row_bytes, e->stream));       // rows from the count on: exactly 0.0
        if (n_mol > 0) {
            HIP_TRY(hipMemcpyAsync(e->d_items.p, h_items.back().data(), h_items.back().size(), hipMemcpyHostToDevice, e->stream));
            const int n_work = n_it * nsplit;
            const int grid = std::max(1, std::min((n_work + kPairWaves - 1) / kPairWaves, e->n_cu * e->pair_blocks_per_cu));
            with_bools([&](auto tri) {
                hipLaunchKernelGGL((molen_sweep_kernel<decltype(tri)::value>), dim3(grid), dim3(kPairBlock), e->coul_bytes, e->stream, tp,
                                   e->bx, (const double *)e->d_pos, (const int *)e->d_nmol, (const double *)e->d_res_q,
                                   (const int *)e->d_res_atype, (const double2 *)e->d_pair_tab, (const char *)e->d_coul_tab,
                                   (const EpItem *)e->d_items.p, nsplit, n_work, (double2 *)e->d_partials.p);
            }, e->bx.triclinic != 0);
            hipLaunchKernelGGL(pair_finalize_kernel, dim3((n_it + 255) / 256), dim3(256), 0, e->stream, (const double2 *)e->d_partials.p,
                               n_it, nsplit, d_lj, d_c);
            if ((rc = launch_intra(e, e->lanes[0], (const PairItem *)((const char *)e->d_items.p + (size_t)n_it * sizeof(EpItem)), n_mol,
                                   nullptr, 1, d_in)))
                return rc;
            double2 *d_tab = (double2 *)e->lanes[0].d_scratch.p, *d_S = d_tab + (size_t)c * tab_n;
            if (any_charged && (rc = launch_sfactor_replicas(e, d_idx, c, d_tab, false, d_S))) return rc;
            hipLaunchKernelGGL(molen_recip_kernel, dim3(n_mol), dim3(kBlock), recip_lds, e->stream, tp, e->bx, (const double *)e->d_kw,
                               (const int *)e->d_kpack, (const int *)e->d_kslot, (const double *)e->d_atom_q, d_recs, tab_n,
                               (const double2 *)d_tab, (const double2 *)d_S, d_u);
        }
        if (n_mol > 0 || bins)
            hipLaunchKernelGGL(molen_reduce_kernel, dim3((n_mol + (bins ? c : 0) + 63) / 64), dim3(64), 0, e->stream, n_res, d_recs, n_mol,
                               d_idx, c, (const double *)d_lj, (const double *)d_c, (const double *)d_in, (const double *)d_u, rows,
                               out ? d_rows : nullptr, bins ? *bins : no_bins, bins ? accum_seg(e->molen.acc, e->molen.d_acc, 0) : nullptr,
                               bins ? accum_seg(e->molen.acc, e->molen.d_acc, 1) : nullptr);
        HIP_TRY(hipGetLastError());
        if (out) HIP_TRY(hipMemcpyAsync(out + (size_t)p.first * rows * 5, d_rows, (size_t)c * row_bytes, hipMemcpyDeviceToHost, e->stream));
    }
    return sync_stream(e);
}

// the replica list of an mgpu_molecule_energy_* call, then "configured": in this order
static int molen_ready(const mgpu_engine *e, int n, const int *replicas, const char *who) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    const int rc = check_index_list(n, replicas, e->n_replicas, "replica", who);
    if (rc) return rc;
    if (e->molen.n_sel == 0)
        return set_error(MGPU_ERR_STATE, std::string(who) + ": no histogram is configured (mgpu_molecule_energy_configure)");
    return MGPU_OK;
}

}  // namespace mgpu

extern "C" {

int mgpu_molecule_energies_replicas(mgpu_engine *e, int n, const int *replicas, int chunk, int n_sel, const int *types, double *out,
                                    int *counts) {
    const char *who = "molecule_energies_replicas";
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = check_index_list(n, replicas, e->n_replicas, "replica", who);
    if (rc) return rc;
    if ((rc = molen_check_types(e, n_sel, types, who))) return rc;
    if (n > 0 && (!out || !counts)) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": null out or counts");
    if (n == 0) return MGPU_OK;
    return molen_passes(e, n, replicas, chunk, n_sel, types, out, counts, nullptr, who);
}

int mgpu_molecule_energy_configure(mgpu_engine *e, int n_bins, double e_min, double e_max, int n_sel, const int *types) {
    const char *who = "molecule_energy_configure";
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc;
    auto &me = e->molen;
    if (n_sel == 0) {
        if ((rc = use_device(e))) return rc;
        if ((rc = sync_all_lanes(e))) return rc;
        me.d_acc.release();
        me.n_sel = 0; me.n_bins = 0;
        return MGPU_OK;
    }
    if (n_bins < 1 || n_bins > kMolenMaxBins)
        return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": n_bins " + std::to_string(n_bins) + " is outside [1, " +
                         std::to_string(kMolenMaxBins) + "]");
    if (!std::isfinite(e_min) || !std::isfinite(e_max) || !(e_min < e_max))
        return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": e_min and e_max must be finite, e_min below e_max");
    if ((rc = molen_check_types(e, n_sel, types, who))) return rc;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    me.d_acc.release();
    me.n_sel = 0;
    const Accum acc = accum_layout((size_t)e->n_replicas, (size_t)n_sel * (n_bins + 2), 1);      // hist | samples
    if ((rc = me.d_acc.reserve(acc.bytes()))) return rc;
    HIP_TRY(hipMemset(me.d_acc.p, 0, acc.bytes()));
    me.acc = acc;
    me.n_bins = n_bins; me.n_sel = n_sel;
    me.e_min = e_min; me.e_max = e_max; me.inv_w = (double)n_bins / (e_max - e_min);
    for (int s = 0; s < n_sel; ++s) me.types[s] = types[s];
    return MGPU_OK;
}

int mgpu_molecule_energy_accumulate_replicas(mgpu_engine *e, int n, const int *replicas, int chunk) {
    const char *who = "molecule_energy_accumulate_replicas";
    int rc = molen_ready(e, n, replicas, who);
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    const auto &me = e->molen;
    const MolenBins bins{me.n_bins, me.n_sel, me.e_min, me.e_max, me.inv_w};
    return molen_passes(e, n, replicas, chunk, me.n_sel, me.types, nullptr, nullptr, &bins, who);
}

int mgpu_molecule_energy_read(mgpu_engine *e, int n, const int *replicas, unsigned long long *hist, unsigned long long *samples) {
    int rc = molen_ready(e, n, replicas, "molecule_energy_read");
    if (rc) return rc;
    if (n > 0 && (!hist || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "molecule_energy_read: null output");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    unsigned long long *const host[3] = {hist, samples, nullptr};
    return accum_read(e->molen.acc, e->molen.d_acc, n, replicas, host, true);
}

int mgpu_molecule_energy_load(mgpu_engine *e, int n, const int *replicas, const unsigned long long *hist,
                              const unsigned long long *samples) {
    int rc = molen_ready(e, n, replicas, "molecule_energy_load");
    if (rc) return rc;
    if (n > 0 && (!hist || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "molecule_energy_load: null input");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const unsigned long long *const host[3] = {hist, samples, nullptr};
    return accum_load(e->molen.acc, e->molen.d_acc, n, replicas, host);
}

int mgpu_molecule_energy_reset(mgpu_engine *e, int n, const int *replicas) {
    int rc = molen_ready(e, n, replicas, "molecule_energy_reset");
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    return accum_reset(e->molen.acc, e->molen.d_acc, n, replicas);
}

int mgpu_system_energy_replicas(mgpu_engine *e, int n, const int *replicas, int chunk, double *out, double *a_deviation) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = check_index_list(n, replicas, e->n_replicas, "replica", "system_energy_replicas");
    if (rc) return rc;
    if (n > 0 && !out) return set_error(MGPU_ERR_INVALID_ARG, "system_energy_replicas: null out");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const Topo &tp = e->tp;
    const int nsplit = e->pair_nsplit;
    const size_t tab_n = phase_tab_entries(e);
    unsigned active_mask = 0;
    SelfTerms self{};
    for (int t = 0; t < tp.n_res; ++t) {
        if (e->is_active[t] == 1) active_mask |= 1u << t;
        self.v[t] = self_energy_host(e, t);
    }
    auto counts = [&](int i, long long &n_pair, long long &n_in) {
        n_pair = 0; n_in = 0;
        for (int t = 0; t < tp.n_res; ++t) {
            const int nm = e->h_nmol[replicas[i] * tp.n_res + t];
            n_pair += nm;
            if (e->is_active[t] == 1) n_in += nm;
        }
    };
    // what a replica adds to a pass: its phase tables and S(k), its items, their split partials and results, its records
    auto bytes_of = [&](long long n_pair, long long n_in) {
        return (tab_n + e->n_slots) * sizeof(double2) + (size_t)(n_pair + n_in) * sizeof(PairItem) +
               (size_t)n_pair * nsplit * sizeof(double2) + (size_t)(2 * n_pair + n_in + 1) * sizeof(double) + sizeof(RecipItem) +
               sizeof(EnergyRep) + sizeof(int);
    };
    std::vector<Pass> passes;
    if (!plan_passes(n, counts, bytes_of, chunk, nsplit, passes))
        return set_error(MGPU_ERR_CAPACITY, "system_energy_replicas: one replica's pair sweep exceeds 2^31 work units");
    size_t max_tab = 0, max_items = 0, max_rec = 0, max_res = 0;
    for (const Pass &p : passes) {
        max_tab = std::max(max_tab, (size_t)p.c * (tab_n + e->n_slots) * sizeof(double2));
        max_items = std::max(max_items, (size_t)(p.n_pair + p.n_in) * sizeof(PairItem));
        max_rec = std::max(max_rec, (size_t)p.c * (sizeof(RecipItem) + sizeof(EnergyRep) + sizeof(int)));
        max_res = std::max(max_res, (size_t)(2 * p.n_pair + p.n_in + p.c) * sizeof(double));
    }
    // every block is reserved once, before the first pass: nothing is freed under a pass still in flight
    const size_t head = (size_t)n * (a_deviation ? 7 : 6) * sizeof(double);
    if ((rc = e->d_out.reserve(head + max_res))) return rc;
    if ((rc = e->d_items.reserve(std::max<size_t>(max_items, 8)))) return rc;
    if ((rc = e->d_items2.reserve(max_rec))) return rc;
    if ((rc = e->lanes[0].d_scratch.reserve(max_tab))) return rc;
    double *d_out6 = (double *)e->d_out.p, *d_dev = d_out6 + (size_t)n * 6, *d_res = (double *)((char *)e->d_out.p + head);
    // the host images of the passes' uploads live until the stream has been waited for
    std::deque<std::vector<PairItem>> h_items;
    std::deque<std::vector<char>> h_recs;
    for (const Pass &p : passes) {
        const int c = p.c, n_pair = (int)p.n_pair, n_in = (int)p.n_in;
        // ComputePairwiseEnergy (energy_utils.f90:83-115): one ordered item per molecule; behind them the intra items of the
        // ACTIVE types (energy_utils.f90:67-69), both replica by replica in (type, molecule) order
        h_items.emplace_back();
        std::vector<PairItem> &items = h_items.back();
        items.reserve((size_t)n_pair + n_in);
        h_recs.emplace_back((size_t)c * (sizeof(RecipItem) + sizeof(EnergyRep) + sizeof(int)));
        char *blob = h_recs.back().data();
        RecipItem *rits = (RecipItem *)blob;
        EnergyRep *reps = (EnergyRep *)(blob + (size_t)c * sizeof(RecipItem));
        int *idx = (int *)(blob + (size_t)c * (sizeof(RecipItem) + sizeof(EnergyRep)));
        int in_at = 0;
        for (int i = 0; i < c; ++i) {
            const int r = replicas[p.first + i];
            EnergyRep &er = reps[i];
            er = EnergyRep{};
            er.replica = r;
            er.pair_first = (int)items.size();
            er.intra_first = in_at;
            for (int t = 0; t < tp.n_res; ++t) {
                er.n[t] = e->h_nmol[r * tp.n_res + t];
                for (int m = 0; m < er.n[t]; ++m) items.push_back(PairItem{r, t, m, -1, 1});
                if (e->is_active[t] == 1) in_at += er.n[t];
            }
            rits[i] = RecipItem{i, 0, -1, MGPU_NONE, -1, 0};       // block i of the pass's S(k): the energy of A as it is
            idx[i] = r;
        }
        for (int i = 0; i < c; ++i)
            for (int t = 0; t < tp.n_res; ++t) {
                if (e->is_active[t] != 1) continue;
                for (int m = 0; m < reps[i].n[t]; ++m) items.push_back(PairItem{reps[i].replica, t, m, -1, 0});
            }
        HIP_TRY(hipMemcpyAsync(e->d_items2.p, blob, h_recs.back().size(), hipMemcpyHostToDevice, e->stream));
        const RecipItem *d_rits = (const RecipItem *)e->d_items2.p;
        const EnergyRep *d_reps = (const EnergyRep *)((const char *)e->d_items2.p + (size_t)c * sizeof(RecipItem));
        const int *d_idx = (const int *)((const char *)e->d_items2.p + (size_t)c * (sizeof(RecipItem) + sizeof(EnergyRep)));
        double *d_lj = d_res, *d_c = d_lj + n_pair, *d_in = d_c + n_pair, *d_u = d_in + n_in;
        if (n_pair > 0) {
            HIP_TRY(hipMemcpyAsync(e->d_items.p, items.data(), items.size() * sizeof(PairItem), hipMemcpyHostToDevice, e->stream));
            if ((rc = launch_pair(e, e->lanes[0], (const PairItem *)e->d_items.p, n_pair, 0, 1, nsplit, d_lj, d_c, true))) return rc;
            if (n_in > 0 && (rc = launch_intra(e, e->lanes[0], (const PairItem *)e->d_items.p + n_pair, n_in, nullptr, 1, d_in))) return rc;
        }
        // ComputeEwaldRecip (energy_utils.f90:270-286): S(k) of every replica of the pass into scratch (the slots no k owns
        // stay zero, as the engine's one-replica scratch keeps them), then sum ff W |S|^2, one item per replica
        double2 *d_tab = (double2 *)e->lanes[0].d_scratch.p, *d_S = d_tab + (size_t)c * tab_n;
        HIP_TRY(hipMemsetAsync(d_S, 0, (size_t)c * e->n_slots * sizeof(double2), e->stream));
        if ((rc = launch_sfactor_replicas(e, d_idx, c, d_tab, false, d_S))) return rc;
        if ((rc = launch_recip(e, e->lanes[0], d_rits, c, 1, 1, false, d_S, d_u))) return rc;
        hipLaunchKernelGGL(energy_reduce_replicas_kernel, dim3((c + 63) / 64), dim3(64), 0, e->stream, tp.n_res, d_reps, c, active_mask,
                           self, (const double *)d_lj, (const double *)d_c, (const double *)d_in, (const double *)d_u,
                           d_out6 + (size_t)p.first * 6);
        if (a_deviation)
            hipLaunchKernelGGL(a_deviation_replicas_kernel, dim3(c), dim3(kBlock), 0, e->stream, e->bx, e->d_kslot, d_idx,
                               (const double2 *)e->d_A, (const double2 *)d_S, d_dev + p.first);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(out, d_out6, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (a_deviation) HIP_TRY(hipMemcpyAsync(a_deviation, d_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    return sync_stream(e);
}

int mgpu_init_structure_factor_replicas(mgpu_engine *e, int n, const int *replicas, int mode) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = check_index_list(n, replicas, e->n_replicas, "replica", "init_structure_factor_replicas");
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    if (mode == 0) {
        // runs of consecutive replicas are zeroed together
        std::vector<int> sorted(replicas, replicas + n);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 0; i < n;) {
            int j = i + 1;
            while (j < n && sorted[j] == sorted[j - 1] + 1) ++j;
            HIP_TRY(hipMemsetAsync(e->d_A + (size_t)sorted[i] * e->n_slots, 0, (size_t)(j - i) * e->n_slots * sizeof(double2), e->stream));
            i = j;
        }
        return sync_stream(e);
    }
    const size_t tab_n = phase_tab_entries(e);
    const int per_pass = (int)std::max<size_t>(1, std::min<size_t>(kReplicasPassMax, kReplicasPassBytes / (tab_n * sizeof(double2))));
    if ((rc = e->d_items2.reserve((size_t)n * sizeof(int)))) return rc;
    if ((rc = e->lanes[0].d_scratch.reserve((size_t)std::min(n, per_pass) * tab_n * sizeof(double2)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items2.p, replicas, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
    for (int first = 0; first < n; first += per_pass)
        if ((rc = launch_sfactor_replicas(e, (const int *)e->d_items2.p + first, std::min(per_pass, n - first),
                                          (double2 *)e->lanes[0].d_scratch.p, true, e->d_A)))
            return rc;
    return sync_stream(e);
}

int mgpu_energy_pairs_replicas(mgpu_engine *e, int n, const int *replicas, int chunk, int n_sel, const int *res_a, const int *res_b,
                               double *out) {
    const char *who = "energy_pairs_replicas";
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = check_index_list(n, replicas, e->n_replicas, "replica", who);
    if (rc) return rc;
    const Topo &tp = e->tp;
    const int n_res = tp.n_res;
    if (n_sel < 1 || n_sel > kEpairsMaxSel)
        return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": n_sel " + std::to_string(n_sel) + " pairs is outside [1, " +
                         std::to_string(kEpairsMaxSel) + "]");
    if (!res_a || !res_b) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": null pair list");
    int sel_a[kEpairsMaxSel], sel_b[kEpairsMaxSel];
    bool taken[kMaxRes][kMaxRes] = {};
    for (int p = 0; p < n_sel; ++p) {
        const int a = std::min(res_a[p], res_b[p]), b = std::max(res_a[p], res_b[p]);
        const std::string name = ": pair " + std::to_string(p) + " (" + std::to_string(res_a[p]) + ", " + std::to_string(res_b[p]) + ")";
        if (a < 0 || b >= n_res)
            return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + name + ": residue type out of range [0, " + std::to_string(n_res - 1) + "]");
        if (taken[a][b]) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + name + " is a duplicate");
        taken[a][b] = true;
        sel_a[p] = a; sel_b[p] = b;
    }
    if (n > 0 && !out) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": null out");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const int nsplit = e->pair_nsplit;
    const int nk = e->nk;
    const size_t tab_n = phase_tab_entries(e);
    // the residue types whose S_t(k) a pass forms: those of the selection with a charged site (the others give exactly 0)
    EpTypes types{};
    int s_index[kMaxRes];
    for (int t = 0; t < n_res; ++t) {
        s_index[t] = -1;
        bool wanted = false, charged = false;
        for (int p = 0; p < n_sel; ++p) wanted = wanted || sel_a[p] == t || sel_b[p] == t;
        for (int a = 0; a < tp.n1[t]; ++a) charged = charged || std::fabs(e->charges[(size_t)t * tp.max_atom + a]) >= kErrorTol;
        if (wanted && charged) { s_index[t] = types.n; types.t[types.n++] = t; }
    }
    // the side of a pair whose molecules are the items: the type of fewer sites (a for equal counts): a guest's molecules
    // against a framework, not the framework against every guest.  Fixed by (a, b) and the topology.
    int item_t[kEpairsMaxSel], part_t[kEpairsMaxSel];
    for (int p = 0; p < n_sel; ++p) {
        const bool a_side = tp.n1[sel_a[p]] <= tp.n1[sel_b[p]];
        item_t[p] = a_side ? sel_a[p] : sel_b[p];
        part_t[p] = a_side ? sel_b[p] : sel_a[p];
    }
    auto counts = [&](int i, long long &n_it, long long &n_in) {
        const int r = replicas[i];
        n_it = 0; n_in = 0;
        for (int p = 0; p < n_sel; ++p) {
            n_it += e->h_nmol[r * n_res + item_t[p]];
            if (sel_a[p] == sel_b[p] && e->is_active[sel_a[p]] == 1) n_in += e->h_nmol[r * n_res + sel_a[p]];
        }
    };
    const size_t s_n = types.n ? tab_n + (size_t)types.n * nk : 0;     // complex entries of a replica's tables and S_t(k)
    auto bytes_of = [&](long long n_it, long long n_in) {
        return s_n * sizeof(double2) + (size_t)n_it * sizeof(EpItem) + (size_t)n_in * sizeof(PairItem) +
               (size_t)n_it * nsplit * sizeof(double2) + (size_t)(2 * n_it + n_in + n_sel) * sizeof(double) +
               (size_t)n_sel * sizeof(EpRec) + sizeof(int);
    };
    std::vector<Pass> passes;
    if (!plan_passes(n, counts, bytes_of, chunk, nsplit, passes))
        return set_error(MGPU_ERR_CAPACITY, std::string(who) + ": one replica's sweep exceeds 2^31 work units");
    size_t max_tab = 0, max_items = 0, max_rec = 0, max_res = 0, max_part = 0;
    for (const Pass &p : passes) {
        max_tab = std::max(max_tab, (size_t)p.c * s_n * sizeof(double2));
        max_items = std::max(max_items, (size_t)p.n_pair * sizeof(EpItem) + (size_t)p.n_in * sizeof(PairItem));
        max_rec = std::max(max_rec, (size_t)p.c * ((size_t)n_sel * sizeof(EpRec) + sizeof(int)));
        max_res = std::max(max_res, (size_t)(2 * p.n_pair + p.n_in + (long long)p.c * n_sel) * sizeof(double));
        max_part = std::max(max_part, (size_t)p.n_pair * nsplit * sizeof(double2));
    }
    // every block is reserved once, before the first pass: nothing is freed under a pass still in flight
    const size_t head = (size_t)n * n_sel * 5 * sizeof(double);
    if ((rc = e->d_out.reserve(head + max_res))) return rc;
    if ((rc = e->d_items.reserve(std::max<size_t>(max_items, 8)))) return rc;
    if ((rc = e->d_items2.reserve(max_rec))) return rc;
    if ((rc = e->d_partials.reserve(std::max<size_t>(max_part, 16)))) return rc;
    if ((rc = e->lanes[0].d_scratch.reserve(std::max<size_t>(max_tab, 16)))) return rc;
    double *d_out5 = (double *)e->d_out.p, *d_res = (double *)((char *)e->d_out.p + head);
    // the host images of the passes' uploads live until the stream has been waited for
    std::deque<std::vector<char>> h_items, h_recs;
    for (const Pass &p : passes) {
        const int c = p.c, n_it = (int)p.n_pair, n_in = (int)p.n_in, n_rec = c * n_sel;
        h_items.emplace_back((size_t)n_it * sizeof(EpItem) + (size_t)n_in * sizeof(PairItem));
        EpItem *items = (EpItem *)h_items.back().data();
        PairItem *in_items = (PairItem *)(h_items.back().data() + (size_t)n_it * sizeof(EpItem));
        h_recs.emplace_back((size_t)n_rec * sizeof(EpRec) + (size_t)c * sizeof(int));
        EpRec *recs = (EpRec *)h_recs.back().data();
        int *idx = (int *)(h_recs.back().data() + (size_t)n_rec * sizeof(EpRec));
        int at = 0, in_at = 0;
        for (int i = 0; i < c; ++i) {
            const int r = replicas[p.first + i];
            idx[i] = r;
            for (int q = 0; q < n_sel; ++q) {
                const int a = sel_a[q], b = sel_b[q];
                EpRec &er = recs[i * n_sel + q];
                er = EpRec{};
                er.entry = i;
                er.same = a == b ? 1 : 0;
                er.sa = s_index[a]; er.sb = s_index[b];
                er.item_first = at;
                er.n_items = e->h_nmol[r * n_res + item_t[q]];
                for (int m = 0; m < er.n_items; ++m) items[at++] = EpItem{r, item_t[q], m, part_t[q]};
                er.intra_first = in_at;
                if (a == b) {
                    er.n_self = e->h_nmol[r * n_res + a];
                    er.self_v = self_energy_host(e, a);
                    if (e->is_active[a] == 1) {
                        // ComputeTotalIntraResidueCoulombEnergy skips the inactive types
                        er.n_intra = er.n_self;
                        for (int m = 0; m < er.n_intra; ++m) in_items[in_at++] = PairItem{r, a, m, -1, 0};
                    }
                }
            }
        }
        HIP_TRY(hipMemcpyAsync(e->d_items2.p, h_recs.back().data(), h_recs.back().size(), hipMemcpyHostToDevice, e->stream));
        const EpRec *d_recs = (const EpRec *)e->d_items2.p;
        const int *d_idx = (const int *)((const char *)e->d_items2.p + (size_t)n_rec * sizeof(EpRec));
        double *d_lj = d_res, *d_c = d_lj + n_it, *d_in = d_c + n_it, *d_u = d_in + n_in;
        if (!h_items.back().empty())
            HIP_TRY(hipMemcpyAsync(e->d_items.p, h_items.back().data(), h_items.back().size(), hipMemcpyHostToDevice, e->stream));
        if (n_it > 0) {
            const int n_work = n_it * nsplit;
            const int grid = std::max(1, std::min((n_work + kPairWaves - 1) / kPairWaves, e->n_cu * e->pair_blocks_per_cu));
            with_bools([&](auto tri) {
                hipLaunchKernelGGL((epairs_sweep_kernel<decltype(tri)::value>), dim3(grid), dim3(kPairBlock), e->coul_bytes, e->stream, tp,
                                   e->bx, (const double *)e->d_pos, (const int *)e->d_nmol, (const double *)e->d_res_q,
                                   (const int *)e->d_res_atype, (const double2 *)e->d_pair_tab, (const char *)e->d_coul_tab,
                                   (const EpItem *)e->d_items.p, nsplit, n_work, (double2 *)e->d_partials.p);
            }, e->bx.triclinic != 0);
            hipLaunchKernelGGL(pair_finalize_kernel, dim3((n_it + 255) / 256), dim3(256), 0, e->stream, (const double2 *)e->d_partials.p,
                               n_it, nsplit, d_lj, d_c);
        }
        if (n_in > 0 && (rc = launch_intra(e, e->lanes[0], (const PairItem *)((const char *)e->d_items.p + (size_t)n_it * sizeof(EpItem)),
                                           n_in, nullptr, 1, d_in)))
            return rc;
        double2 *d_tab = (double2 *)e->lanes[0].d_scratch.p, *d_S = d_tab + (size_t)c * tab_n;
        if (types.n > 0) {
            launch_phase_tables_replicas(e, d_idx, c, d_tab);
            hipLaunchKernelGGL(sfactor_types_replicas_kernel, dim3(nk, c), dim3(kBlock), 0, e->stream, tp, e->bx, (const int *)e->d_nmol,
                               (const int *)e->d_atom_mol, (const double *)e->d_atom_q, (const int *)e->d_kpack, d_idx, tab_n,
                               (const double2 *)d_tab, types, d_S);
        }
        hipLaunchKernelGGL(epairs_recip_kernel, dim3(n_rec), dim3(kBlock), 0, e->stream, e->bx, (const double *)e->d_kw, d_recs,
                           types.n, (const double2 *)d_S, d_u);
        hipLaunchKernelGGL(epairs_reduce_kernel, dim3((n_rec + 63) / 64), dim3(64), 0, e->stream, d_recs, n_rec, (const double *)d_lj,
                           (const double *)d_c, (const double *)d_in, (const double *)d_u, d_out5 + (size_t)p.first * n_sel * 5);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(out, d_out5, head, hipMemcpyDeviceToHost, e->stream));
    return sync_stream(e);
}

int mgpu_rdf_configure(mgpu_engine *e, int n_bins, double r_max, int n_pairs, const int *type_a, const int *type_b, int include_intra) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc;
    if (n_pairs == 0) {
        if ((rc = use_device(e))) return rc;
        if ((rc = sync_all_lanes(e))) return rc;
        e->rdf.d_acc.release();
        e->rdf.d_tab.release();
        e->rdf.n_pairs = 0; e->rdf.n_bins = 0;
        return MGPU_OK;
    }
    if (n_bins < 1 || n_bins > kRdfMaxBins)
        return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: n_bins " + std::to_string(n_bins) + " is outside [1, " + std::to_string(kRdfMaxBins) + "]");
    if (n_pairs < 1 || n_pairs > kRdfMaxPairs)
        return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: n_pairs " + std::to_string(n_pairs) + " is outside [1, " + std::to_string(kRdfMaxPairs) + "]");
    if (!type_a || !type_b) return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: null pair list");
    if (include_intra != 0 && include_intra != 1) return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: include_intra must be 0 or 1");
    if (!(r_max > 0.0) || !std::isfinite(r_max)) return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: r_max must be greater than 0");
    const double limit = rdf_half_width(e);
    if (r_max > limit)
        return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: r_max " + rdf_number(r_max) +
                         " exceeds half the smallest perpendicular width of the cell, " + rdf_number(limit));
    const int nt = e->tp.n_types;
    RdfTable tab;
    for (int a = 0; a < kMaxTypes; ++a) { tab.row[a] = ~0ull; tab.partner[a] = 0; }
    for (int p = 0; p < n_pairs; ++p) {
        const int a = type_a[p], b = type_b[p];
        if (a < 0 || a >= nt || b < 0 || b >= nt || a >= kMaxTypes || b >= kMaxTypes)
            return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: pair " + std::to_string(p) + ": atom type out of range [0, " +
                             std::to_string(nt - 1) + "]");
        if (nibble_get(tab.row[a], b) != kNibbleNone)
            return set_error(MGPU_ERR_INVALID_ARG, "rdf_configure: pair " + std::to_string(p) + " (" + std::to_string(a) + ", " +
                             std::to_string(b) + ") is a duplicate");
        tab.row[a] = nibble_set(tab.row[a], b, (unsigned)p);
        tab.row[b] = nibble_set(tab.row[b], a, (unsigned)p);
        tab.partner[a] |= 1u << b;
        tab.partner[b] |= 1u << a;
    }
    // a workgroup's 32-bit LDS bins take at most 256 x (atom slots) counts, its molecule keys (type << 28) | molecule
    if (e->tp.n_cap_atoms >= (1 << 24))
        return set_error(MGPU_ERR_CAPACITY, "rdf_configure: more than 2^24 atom slots per replica");
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    e->rdf.d_acc.release();
    e->rdf.n_pairs = 0;
    const Accum acc = accum_layout((size_t)e->n_replicas, (size_t)n_pairs * n_bins, (size_t)n_pairs, 1);   // hist | eligible | samples
    if ((rc = e->rdf.d_acc.reserve(acc.bytes()))) return rc;
    if ((rc = e->rdf.d_tab.reserve(sizeof(RdfTable)))) return rc;
    HIP_TRY(hipMemset(e->rdf.d_acc.p, 0, acc.bytes()));
    HIP_TRY(hipMemcpy(e->rdf.d_tab.p, &tab, sizeof tab, hipMemcpyHostToDevice));
    e->rdf.acc = acc;
    e->rdf.n_bins = n_bins; e->rdf.n_pairs = n_pairs; e->rdf.include_intra = include_intra;
    e->rdf.r_max = r_max; e->rdf.r_max2 = r_max * r_max; e->rdf.inv_dr = (double)n_bins / r_max;
    for (int p = 0; p < n_pairs; ++p) { e->rdf.type_a[p] = type_a[p]; e->rdf.type_b[p] = type_b[p]; }
    return MGPU_OK;
}

int mgpu_rdf_accumulate_replicas(mgpu_engine *e, int n, const int *replicas, int chunk) {
    int rc = rdf_ready(e, n, replicas, "rdf_accumulate_replicas");
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const Accum &acc = e->rdf.acc;
    if ((rc = e->d_items2.reserve((size_t)n * sizeof(int)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items2.p, replicas, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
    const int most = chunk > 0 ? std::min(chunk, kReplicasPassMax) : kReplicasPassMax;
    const int n_iblk = (e->tp.n_cap_atoms + kRdfBlock - 1) / kRdfBlock;
    const size_t lds = acc.per[0] * sizeof(unsigned);
    for (int first = 0; first < n; first += most) {
        const int c = std::min(most, n - first);
        // j chunks per i block: few replicas -> many chunks, to give every CU some workgroups; many replicas -> one
        RdfArgs ra{e->rdf.n_bins, e->rdf.n_pairs, e->rdf.include_intra, 1, e->rdf.r_max2, e->rdf.inv_dr};
        const long long tiles = (long long)c * n_iblk;
        ra.n_chunk = (int)std::max<long long>(1, std::min<long long>(n_iblk, (4LL * e->n_cu + tiles - 1) / tiles));
        const dim3 grid((unsigned)(n_iblk * ra.n_chunk), (unsigned)c);
        const int *d_reps = (const int *)e->d_items2.p + first;
        with_bools([&](auto tri) {
            hipLaunchKernelGGL((rdf_hist_kernel<decltype(tri)::value>), grid, dim3(kRdfBlock), lds, e->stream, e->tp, e->bx, ra,
                               (const double *)e->d_pos, (const int *)e->d_nmol, (const int *)e->d_atom_res,
                               (const int *)e->d_atom_mol, d_reps, (const RdfTable *)e->rdf.d_tab.p, accum_seg(acc, e->rdf.d_acc, 0),
                               accum_seg(acc, e->rdf.d_acc, 1), accum_seg(acc, e->rdf.d_acc, 2));
        }, e->bx.triclinic != 0);
        HIP_TRY(hipGetLastError());
    }
    return sync_stream(e);
}

int mgpu_rdf_read(mgpu_engine *e, int n, const int *replicas, unsigned long long *hist, unsigned long long *eligible,
                  unsigned long long *samples) {
    int rc = rdf_ready(e, n, replicas, "rdf_read");
    if (rc) return rc;
    if (n > 0 && (!hist || !eligible || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "rdf_read: null output");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    unsigned long long *const host[3] = {hist, eligible, samples};
    return accum_read(e->rdf.acc, e->rdf.d_acc, n, replicas, host, true);
}

int mgpu_rdf_load(mgpu_engine *e, int n, const int *replicas, const unsigned long long *hist, const unsigned long long *eligible,
                  const unsigned long long *samples) {
    int rc = rdf_ready(e, n, replicas, "rdf_load");
    if (rc) return rc;
    if (n > 0 && (!hist || !eligible || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "rdf_load: null input");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const unsigned long long *const host[3] = {hist, eligible, samples};
    return accum_load(e->rdf.acc, e->rdf.d_acc, n, replicas, host);
}

int mgpu_rdf_reset(mgpu_engine *e, int n, const int *replicas) {
    int rc = rdf_ready(e, n, replicas, "rdf_reset");
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    return accum_reset(e->rdf.acc, e->rdf.d_acc, n, replicas);
}

int mgpu_density_configure(mgpu_engine *e, const int *n, int n_channels, const int *types, int n_groups, const int *group_of) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc;
    auto &d = e->density;
    if (n_channels == 0) {
        if ((rc = use_device(e))) return rc;
        if ((rc = sync_all_lanes(e))) return rc;
        d.d_acc.release();
        d.d_group.release();
        d.n_channels = 0; d.n_groups = 0;
        return MGPU_OK;
    }
    if (!n) return set_error(MGPU_ERR_INVALID_ARG, "density_configure: null grid");
    unsigned long long voxels = 1;
    for (int k = 0; k < 3; ++k) {
        if (n[k] < 1 || n[k] > kDensityMaxAxis)
            return set_error(MGPU_ERR_INVALID_ARG, "density_configure: grid axis " + std::to_string(k) + " has " + std::to_string(n[k]) +
                             " voxels, outside [1, " + std::to_string(kDensityMaxAxis) + "]");
        voxels *= (unsigned long long)n[k];
    }
    if (voxels > (unsigned long long)kDensityMaxVoxels)
        return set_error(MGPU_ERR_INVALID_ARG, "density_configure: a grid of " + std::to_string(voxels) + " voxels exceeds the limit of " +
                         std::to_string(kDensityMaxVoxels));
    if (n_channels < 1 || n_channels > kDensityMaxChannels)
        return set_error(MGPU_ERR_INVALID_ARG, "density_configure: n_channels " + std::to_string(n_channels) + " is outside [1, " +
                         std::to_string(kDensityMaxChannels) + "]");
    if (!types) return set_error(MGPU_ERR_INVALID_ARG, "density_configure: null type list");
    const int nt = e->tp.n_types;
    unsigned long long table = ~0ull;
    for (int c = 0; c < n_channels; ++c) {
        const int t = types[c];
        if (t < 0 || t >= nt || t >= kMaxTypes)
            return set_error(MGPU_ERR_INVALID_ARG, "density_configure: channel " + std::to_string(c) + ": atom type out of range [0, " +
                             std::to_string(nt - 1) + "]");
        if (nibble_get(table, t) != kNibbleNone)
            return set_error(MGPU_ERR_INVALID_ARG, "density_configure: channel " + std::to_string(c) + " (atom type " + std::to_string(t) +
                             ") is a duplicate");
        table = nibble_set(table, t, (unsigned)c);
    }
    const int R = e->n_replicas;
    if (n_groups < 1 || n_groups > R)
        return set_error(MGPU_ERR_INVALID_ARG, "density_configure: n_groups " + std::to_string(n_groups) + " is outside [1, " +
                         std::to_string(R) + "]");
    if (!group_of) return set_error(MGPU_ERR_INVALID_ARG, "density_configure: null group_of");
    for (int r = 0; r < R; ++r)
        if (group_of[r] < -1 || group_of[r] >= n_groups)
            return set_error(MGPU_ERR_INVALID_ARG, "density_configure: replica " + std::to_string(r) + ": group " + std::to_string(group_of[r]) +
                             " is outside [0, " + std::to_string(n_groups - 1) + "] and not -1");
    // (2^24 voxels x 8 channels x 2^31 groups x 8 bytes stays below 2^64)
    const Accum acc = accum_layout((size_t)n_groups, (size_t)n_channels * voxels, 1);       // hist | samples
    const unsigned long long bytes = acc.bytes();
    if (bytes > MGPU_DENSITY_MAX_BYTES)
        return set_error(MGPU_ERR_INVALID_ARG, "density_configure: the accumulators would take " + std::to_string(bytes) +
                         " bytes, the limit is " + std::to_string(MGPU_DENSITY_MAX_BYTES));
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    d.d_acc.release();
    d.n_channels = 0; d.n_groups = 0;
    HIP_TRY(hipMalloc(&d.d_acc.p, (size_t)bytes));             // exactly: a map may be large
    d.d_acc.bytes = (size_t)bytes;
    if ((rc = d.d_group.reserve((size_t)R * sizeof(int)))) return rc;
    HIP_TRY(hipMemset(d.d_acc.p, 0, (size_t)bytes));
    HIP_TRY(hipMemcpy(d.d_group.p, group_of, (size_t)R * sizeof(int), hipMemcpyHostToDevice));
    for (int k = 0; k < 3; ++k) d.n[k] = n[k];
    for (int c = 0; c < n_channels; ++c) d.types[c] = types[c];
    d.table = table;
    d.acc = acc;
    d.n_channels = n_channels; d.n_groups = n_groups;
    return MGPU_OK;
}

int mgpu_density_accumulate_replicas(mgpu_engine *e, int n, const int *replicas, int chunk) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = check_index_list(n, replicas, e->n_replicas, "replica", "density_accumulate_replicas");
    if (rc) return rc;
    if ((rc = density_ready(e, "density_accumulate_replicas"))) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const auto &d = e->density;
    if ((rc = e->d_items2.reserve((size_t)n * sizeof(int)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items2.p, replicas, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
    const int most = chunk > 0 ? std::min(chunk, kReplicasPassMax) : kReplicasPassMax;
    const int n_blk = (e->tp.n_cap_atoms + kDensityBlock - 1) / kDensityBlock;
    const DensityArgs da{{d.n[0], d.n[1], d.n[2]}, d.n_channels, d.table};
    for (int first = 0; first < n; first += most) {
        const int c = std::min(most, n - first);
        const int *d_reps = (const int *)e->d_items2.p + first;
        with_bools([&](auto tri) {
            hipLaunchKernelGGL((density_map_kernel<decltype(tri)::value>), dim3((unsigned)n_blk, (unsigned)c), dim3(kDensityBlock), 0, e->stream,
                               e->tp, e->bx, da, (const double *)e->d_pos, (const int *)e->d_nmol, (const int *)e->d_atom_res,
                               (const int *)e->d_atom_mol, d_reps, (const int *)d.d_group.p, accum_seg(d.acc, d.d_acc, 0),
                               accum_seg(d.acc, d.d_acc, 1));
        }, e->bx.triclinic != 0);
        HIP_TRY(hipGetLastError());
    }
    return sync_stream(e);
}

int mgpu_density_read(mgpu_engine *e, int n, const int *groups, unsigned long long *hist, unsigned long long *samples) {
    int rc = density_groups_ready(e, n, groups, "density_read");
    if (rc) return rc;
    if (n > 0 && (!hist || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "density_read: null output");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    unsigned long long *const host[3] = {hist, samples, nullptr};
    return accum_read(e->density.acc, e->density.d_acc, n, groups, host, false);       // (a block may be 2 GiB: not as a whole)
}

int mgpu_density_load(mgpu_engine *e, int n, const int *groups, const unsigned long long *hist, const unsigned long long *samples) {
    int rc = density_groups_ready(e, n, groups, "density_load");
    if (rc) return rc;
    if (n > 0 && (!hist || !samples)) return set_error(MGPU_ERR_INVALID_ARG, "density_load: null input");
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    const unsigned long long *const host[3] = {hist, samples, nullptr};
    return accum_load(e->density.acc, e->density.d_acc, n, groups, host);
}

int mgpu_density_reset(mgpu_engine *e, int n, const int *groups) {
    int rc = density_groups_ready(e, n, groups, "density_reset");
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if ((rc = use_device(e))) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    return accum_reset(e->density.acc, e->density.d_acc, n, groups);
}

}  // extern "C"
