// The kernel launches of the engine: pair sweeps (plane by plane, flat, frozen), the reciprocal update (row form, per k),
// the intra-molecular sum and S(k).  Every launch goes to a lane's stream; nothing here synchronises.
#include "mgpu_engine.h"

namespace mgpu {

template <auto Kernel>
int resident_blocks(Lane &ln, size_t dyn_lds) {
    const void *key = (const void *)Kernel;
    for (const auto &o : ln.occ)
        if (o.kernel == key && o.lds == dyn_lds) return o.blocks;
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, Kernel, kPairBlock, dyn_lds) != hipSuccess || v < 1) v = 1;
    ln.occ.push_back({key, dyn_lds, std::min(v, 4)});
    return ln.occ.back().blocks;
}

// launch the pair sweep + finalize for items already on the device; results land in d_lj / d_c.
// common_n1 = number of sites when every item has the same count (register path for <= 4), else 0.
// host_partials != nullptr: the split partials are written there and NOT reduced on the device (the caller
// copies them out with its results and adds them up in the same order on the host: one launch and one
// inter-kernel gap less per batch; d_lj / d_c are unused).
int launch_pair(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, int common_n1, int site_stride,
                int nsplit, double *d_lj, double *d_c, bool ordered, double2 *host_partials, bool fused, bool fast_fold,
                bool skip_frozen) {
    const int n_work = n_items * nsplit;
    int rc = MGPU_OK;
    if (fused && (!host_partials || ordered || e->bx.triclinic || common_n1 < 1 || common_n1 > kMaxFusedSites))
        return set_error(MGPU_ERR_STATE, "launch_pair: fused sweep needs register sites, an orthorhombic box and a partials buffer");
    if (!host_partials && (rc = ln.d_partials.reserve((size_t)n_work * sizeof(double2)))) return rc;
    double2 *d_part = host_partials ? host_partials : (double2 *)ln.d_partials.p;
    // persistent waves: 2 workgroups of 8 waves per CU (VGPRs: 4 waves per SIMD at <= 128), never more
    // workgroups than there is work for
    const int per_cu = e->pair_blocks_per_cu;
    const int grid = std::max(1, std::min((n_work + kPairWaves - 1) / kPairWaves, e->n_cu * per_cu));
    hipEvent_t a = nullptr, b = nullptr;
    rc = prof_begin(e, ln, MGPU_KERNEL_PAIR, &a, &b);
    if (rc) return rc;
    // the sweeps' argument list (the flat kernels take skip_frozen behind it)
    auto launch = [&](auto kernel, int grid_k, auto... tail) {
        hipExtLaunchKernelGGL(kernel, dim3(grid_k), dim3(kPairBlock), e->coul_bytes, ln.stream, a, b, 0, e->tp, e->bx, e->d_pos, e->d_nmol,
                              e->d_res_q, e->d_res_atype, e->d_pair_tab, e->d_coul_tab, d_items, (const double *)ln.d_sites.p, site_stride,
                              nsplit, n_work, d_part, tail...);
    };
    // fast_fold: every atom of the replicas involved lies within one box length of the cell centre (tracked on the
    // host), so the register-site kernels may fold separations with two instructions per axis (image_r2_fast)
    const bool ff = fast_fold && !ordered && !e->bx.triclinic && e->pair_fast_fold;
    // the plane-by-plane sweep with NS register sites, fused or not, either fold
    auto sweep = [&](auto NS, auto FU) {
        with_bools([&](auto FW) { launch(pair_sweep_kernel<decltype(NS)::value, false, false, decltype(FU)::value, decltype(FW)::value>, grid); }, ff);
    };
    // flat kernels: as many workgroups per CU as their registers and the LDS tables allow
    auto flat_sweep = [&](auto NS, auto FU) {
        with_bools([&](auto FW) {
            constexpr auto kernel = &pair_flat_kernel<decltype(NS)::value, decltype(FU)::value, decltype(FW)::value>;
            const int nb = resident_blocks<kernel>(ln, e->coul_bytes);
            launch(kernel, std::max(1, std::min((n_work + kPairWaves - 1) / kPairWaves, e->n_cu * nb)), skip_frozen ? 1 : 0);
        }, ff);
    };
    // (fused items have at most kMaxFusedSites sites: checked above; flat ones at most kMaxFusedSitesWide: `flat`)
    const bool flat = e->pair_flat && !ordered && !e->bx.triclinic && common_n1 >= 1 && common_n1 <= kMaxFusedSitesWide;
    if (flat && fused) {
        with_int<1, kMaxFusedSites>(common_n1, [&](auto NS) { flat_sweep(NS, std::true_type{}); });
    } else if (flat) {
        with_int<1, kMaxFusedSitesWide>(common_n1, [&](auto NS) { flat_sweep(NS, std::false_type{}); });
    } else if (fused) {
        with_int<1, kMaxFusedSites>(common_n1, [&](auto NS) { sweep(NS, std::true_type{}); });
    } else if (e->bx.triclinic) {
        // triclinic boxes, round 5: the register-site sweeps with ComputeDistance's image search (image_r2_tri_lower / the full
        // 27); a move is two single-state items (trial_submit_impl)
        if (ordered) launch(pair_sweep_kernel<0, true, true>, grid);
        else if (!with_int<1, kMaxFusedSitesWide>(common_n1, [&](auto NS) { launch(pair_sweep_kernel<decltype(NS)::value, false, true>, grid); }))
            launch(pair_sweep_kernel<0, false, true>, grid);
    } else if (ordered) {
        launch(pair_sweep_kernel<0, true, false>, grid);
    } else if (!with_int<1, kMaxFusedSitesWide>(common_n1, [&](auto NS) { sweep(NS, std::false_type{}); })) {
        launch(pair_sweep_kernel<0, false, false>, grid);      // mixed site counts, larger molecules: the LDS-staged sweep
    }
    rc = prof_end(e, ln, MGPU_KERNEL_PAIR, a, b);
    if (rc) return rc;
    // (The reduction stays a separate launch: letting the last wave of an item reduce the partials needs
    //  agent-scope fences, and on the 8-XCD part those write back / invalidate the XCD's L2 -- measured:
    //  pair sweep 110 -> 275 us.  Likewise results are copied out once rather than stored by the kernels
    //  into pinned host memory: thousands of 8-byte PCIe writes were 3-7x slower than the blit.)
    if (!host_partials)
        hipLaunchKernelGGL(pair_finalize_kernel, dim3((n_items + 255) / 256), dim3(256), 0, ln.stream,
                           (const double2 *)ln.d_partials.p, n_items, nsplit, d_lj, d_c);
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// Framework atoms per work unit of pair_frozen_kernel: the fewest chunks that are a multiple of the eight waves of a
// workgroup (a workgroup takes eight chunks of one candidate group: no idle wave in the last one) and hold at most 30
// atoms.  Measured at the 2208-atom framework, chunks of 24 / 28 / 32 / 36 / 40 atoms, us per launch with its finalize:
// 1531 evaluations 52.2 / 42.4 / 42.3 / 46.2 / 47.6, 3066: 66.6 / 60.4 / 62.1 / 68.7 / 72.0, 6156: 106.5 / 105.0 / 110.8 /
// 111.2 / 97.6 -> 28 atoms (80 chunk slots, 79 used).
int frozen_chunk_atoms(const mgpu_engine *e, int n_atoms) {
    const int n_slots = kPairWaves * std::max(1, (n_atoms + kPairWaves * 30 - 1) / (kPairWaves * 30));
    return std::max(1, std::min(64, (n_atoms + n_slots - 1) / n_slots));
}

// The framework part of a launch segment, candidates in the lanes (pair_frozen_kernel): items of
// ONE residue type with n1 register sites; one extra record {e_lj, e_coul} per entry lands in d_extra.
int launch_frozen(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, int n1, int site_stride, bool fused, bool fast_fold,
                  int t_frozen, double2 *d_scratch, double2 *d_extra) {
    const int n_atoms = e->h_nmol[t_frozen] * e->tp.n1[t_frozen];
    const int chunk_atoms = frozen_chunk_atoms(e, n_atoms);
    const int n_chunks = (n_atoms + chunk_atoms - 1) / chunk_atoms;
    if (n_chunks == 0 || n_items == 0) return MGPU_OK;
    // one workgroup per (group of 64 candidates, eight chunks): pair_frozen_kernel
    const int n_wg_units = ((n_items + 63) / 64) * ((n_chunks + kPairWaves - 1) / kPairWaves);
    const bool ff = fast_fold && e->pair_fast_fold;
    hipEvent_t a = nullptr, b = nullptr;
    int rc;
    {
        const size_t need = (size_t)((n_items + 63) / 64) * sizeof(int);
        const void *before = ln.d_tickets.p;
        if ((rc = ln.d_tickets.reserve(need))) return rc;
        if (ln.d_tickets.p != before) HIP_TRY(hipMemsetAsync(ln.d_tickets.p, 0, ln.d_tickets.bytes, ln.stream));
    }
    if ((rc = prof_begin(e, ln, MGPU_KERNEL_PAIR, &a, &b))) return rc;
    auto launch = [&](auto NS, auto FU) {
        with_bools([&](auto FW) {
            constexpr auto kernel = &pair_frozen_kernel<decltype(NS)::value, decltype(FU)::value, decltype(FW)::value>;
            const int nb = resident_blocks<kernel>(ln, e->coul_bytes);
            hipExtLaunchKernelGGL(kernel, dim3(std::max(1, std::min(n_wg_units, e->n_cu * nb))), dim3(kPairBlock), e->coul_bytes, ln.stream,
                                  a, b, 0, e->tp, e->bx, e->d_pos, e->d_nmol, e->d_res_q, e->d_res_atype, e->d_pair_tab, e->d_coul_tab,
                                  d_items, (const double *)ln.d_sites.p, site_stride, n_items, t_frozen, n_chunks, chunk_atoms, d_scratch,
                                  (int *)ln.d_tickets.p, d_extra, (const double *)e->d_atom_q_on, (const int *)e->tp.slot_ty);
        }, ff);
    };
    // (fused items have at most kMaxFusedSites sites: trial_submit_impl sends larger molecules' moves as two single-state items)
    if (fused && n1 > kMaxFusedSites) return set_error(MGPU_ERR_STATE, "launch_frozen: fused items have at most three sites");
    const bool took = fused ? with_int<1, kMaxFusedSites>(n1, [&](auto NS) { launch(NS, std::true_type{}); })
                            : with_int<1, kMaxFusedSitesWide>(n1, [&](auto NS) { launch(NS, std::false_type{}); });
    if (!took) return set_error(MGPU_ERR_STATE, "launch_frozen: items of one to five register sites only");
    if ((rc = prof_end(e, ln, MGPU_KERNEL_PAIR, a, b))) return rc;
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// row form while its XY table fits the LDS budget (molecules of a few sites), else the per-k form
bool recip_by_rows(const mgpu_engine *e, int n1_max) {
    return !e->recip_force_per_k && e->n_rtasks > 0 && recip_rows_lds_bytes(e, n1_max) <= kRecipRowsLdsMax;
}

// The wide row form (recip_rows_wide_kernel): the phase tables of every site-state of the largest molecule of the launch
// in LDS, the XY table a tile of rows at a time.  Rows per tile (0: does not apply -- no row structure, or
// recip_wide_rows_per_tile's reasons).
static int wide_rows_per_tile(const mgpu_engine *e, int n1_max) {
    if (e->recip_force_per_k || e->n_rtasks <= 0 || !e->d_row_first) return 0;
    return recip_wide_rows_per_tile(recip_ktot(e), e->n_rrows, n1_max);
}

// The matrix-unit form of the wide row sweep (recip_rows_wide_kernel<..., MFMA>): only the 1-D phase tables of a TILE of
// site-states in LDS.  Site-states per tile (recip_wide_mfma_tile; 0: the form does not apply): one tile for a molecule of a
// few dozen sites; a molecule of any size otherwise, the four sums of a task carried from tile to tile.  (Measured, 1024
// candidates of 128 / 300 sites: tiles of 52-72 KB 147 / 456-466 us, of 100-144 KB -- one workgroup per CU, opted in with
// hipFuncAttributeMaxDynamicSharedMemorySize -- 148-184 / 613-623 us.)
static int wide_mfma_tile(const mgpu_engine *e, int n1_max) {
    if (e->recip_force_per_k || e->recip_no_mfma || e->n_rtasks <= 0 || !e->d_row_first || !e->rows_contiguous) return 0;
    return recip_wide_mfma_tile(recip_ktot(e), e->n_rrows, n1_max);
}

// The kernel launch_recip takes for molecules of up to n1_max sites.  wide_ok = false: a commit by accept mask or the deciding
// sweep, which have the row form only.
RecipPlan recip_plan(const mgpu_engine *e, int n1_max, bool wide_ok) {
    RecipPlan p;
    const int ktot = recip_ktot(e);
    p.by_rows = recip_by_rows(e, n1_max);
    // per-k form: the molecule's sites pass through LDS a tile at a time (recip_kernel), so no molecule is too large;
    // the tile is the most sites whose two table sets fit kRecipTileBytes (a few-site molecule: one tile)
    p.tile = p.by_rows ? n1_max : recip_tile_sites(ktot, n1_max);
    p.lds = p.by_rows ? recip_rows_lds_bytes(e, n1_max) : recip_lds_bytes(ktot, p.tile);
    const bool wide = wide_ok && !p.by_rows;
    p.mfma_tile = wide ? wide_mfma_tile(e, n1_max) : 0;
    p.wide_rpt = (wide && !p.mfma_tile) ? wide_rows_per_tile(e, n1_max) : 0;
    if (p.mfma_tile || p.wide_rpt) {
        // (matrix-unit form: the site-states of one LDS tile, a multiple of four)
        p.wide_nss = p.mfma_tile ? p.mfma_tile : 2 * n1_max;
        p.wide_lds = recip_wide_lds_bytes(ktot, e->n_rrows, p.wide_nss, p.wide_rpt, p.mfma_tile > 0);
    }
    const int nss = ((2 * n1_max + 3) & ~3);
    if (p.by_rows) p.form = MGPU_RECIP_FORM_ROWS;
    else if (p.mfma_tile) p.form = p.mfma_tile < nss ? MGPU_RECIP_FORM_WIDE_MFMA_TILED : MGPU_RECIP_FORM_WIDE_MFMA;
    else if (p.wide_rpt) p.form = MGPU_RECIP_FORM_WIDE_VECTOR;
    else p.form = MGPU_RECIP_FORM_PER_K;
    return p;
}

// Two molecules whose updates run in one launch of the form their types take alone: the same kernel with the same tile
// shape.  Any two row-form types qualify: recip_rows_kernel's sums do not depend on the launch's largest molecule.
static bool same_recip_form(const RecipPlan &a, const RecipPlan &b) {
    if (a.form != b.form) return false;
    switch (a.form) {
        case MGPU_RECIP_FORM_ROWS: return true;
        case MGPU_RECIP_FORM_PER_K: return a.tile == b.tile;
        case MGPU_RECIP_FORM_WIDE_VECTOR: return a.tile == b.tile && a.wide_rpt == b.wide_rpt;
        default: return a.mfma_tile == b.mfma_tile;
    }
}

// The items of a launch by the form of each one's own residue type: groups of one form, items in their
// order within a group.  order[slot] = item; empty when there is one group (every launch of one residue type, every mix of
// row-form types), whose items stay as they are.
void recip_groups(const mgpu_engine *e, const RecipItem *items, int n, std::vector<RecipGroup> &groups, std::vector<int> &order) {
    groups.clear();
    order.clear();
    RecipPlan plan_of[kMaxRes];
    int group_of[kMaxRes];
    bool seen[kMaxRes] = {false};
    std::vector<RecipPlan> group_plan;
    int n1_all = 1;
    for (int c = 0; c < n; ++c) {
        const int t = items[c].t;
        n1_all = std::max(n1_all, e->tp.n1[t]);
        if (seen[t]) continue;
        seen[t] = true;
        plan_of[t] = recip_plan(e, e->tp.n1[t], true);
        int g = 0;
        while (g < (int)groups.size() && !same_recip_form(group_plan[g], plan_of[t])) ++g;
        if (g == (int)groups.size()) { groups.push_back(RecipGroup{0, 0, 1}); group_plan.push_back(plan_of[t]); }
        group_of[t] = g;
        groups[g].n1_max = std::max(groups[g].n1_max, e->tp.n1[t]);
    }
    if (groups.size() <= 1) {
        groups.assign(1, RecipGroup{0, n, n1_all});
        return;
    }
    for (int c = 0; c < n; ++c) groups[group_of[items[c].t]].n += 1;
    for (size_t g = 1; g < groups.size(); ++g) groups[g].first = groups[g - 1].first + groups[g - 1].n;
    order.resize(n);
    std::vector<int> at(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) at[g] = groups[g].first;
    for (int c = 0; c < n; ++c) order[at[group_of[items[c].t]]++] = c;
}

// accept != nullptr (commit, row form only): d_items are the candidates of the lane's last trial and only
// those whose bit is set are applied
int launch_recip(mgpu_engine *e, Lane &ln, const RecipItem *d_items, int n_items, int n1_max, int site_stride,
                 bool commit, double2 *A_base, double *d_u, double *d_u_old, const AcceptBits *accept, const double *sites_override,
                 const DecideArgs *decide, bool store_alt) {
    const RecipPlan plan = recip_plan(e, n1_max, !accept && !decide);
    // the replicas' A(k): each one's current buffer where the engine keeps two (a scratch A(k) such as S(k): as it is)
    const RecipA Ab = (A_base == e->d_A && e->d_acur) ? RecipA{e->d_A, e->d_A_alt, e->d_acur} : RecipA{A_base, nullptr, nullptr};
    if (store_alt && (!plan.by_rows || commit || decide || !d_u_old || !Ab.cur))
        return set_error(MGPU_ERR_STATE, "A + delta into the other buffer needs the row-form old + new k sweep and the double buffer");
    const bool by_rows = plan.by_rows;
    const double *d_cand = sites_override ? sites_override : (const double *)ln.d_sites.p;
    static const AcceptBits no_bits{};
    const AcceptBits &bits = accept ? *accept : no_bits;
    if (accept && !by_rows) return set_error(MGPU_ERR_STATE, "commit by accept mask needs the row-form kernel");
    if (decide && (!by_rows || commit || !d_u_old)) return set_error(MGPU_ERR_STATE, "device-side acceptance needs the row-form old + new k sweep");
    const DecideArgs no_decide{};
    if (plan.lds > kLdsDefaultMax)
        return set_error(MGPU_ERR_CAPACITY, "reciprocal update: kmax too large for the LDS phase tables (" +
                                                std::to_string(plan.lds) + " B > 64 KiB for one site)");
    hipEvent_t a = nullptr, b = nullptr;
    const int slot = commit ? MGPU_KERNEL_COMMIT : MGPU_KERNEL_RECIP;
    int rc = prof_begin(e, ln, slot, &a, &b);
    if (rc) return rc;
    // what a sweep does, as its kernels' <COMMIT, BOTH>: the new state's energy; that and the energy of the unchanged A(k) from
    // the same pass (d_u_old, trial moves); the commit
    auto with_pass = [&](auto &&f) {
        if (commit) f(std::true_type{}, std::false_type{});
        else with_bools([&](auto BOTH) { f(std::false_type{}, BOTH); }, d_u_old != nullptr);
    };
    // recip_rows_kernel's argument list
    auto rows = [&](auto kernel, int use_accept, const DecideArgs &da) {
        hipExtLaunchKernelGGL(kernel, dim3(n_items), dim3(kBlock), plan.lds, ln.stream, a, b, 0, e->tp, e->bx, e->d_pos, e->d_nmol, e->d_res_q,
                              e->d_trj, e->d_tw, e->n_rtasks, e->d_rrows, e->n_rrows, Ab, d_items, d_cand, site_stride, d_u, d_u_old, bits,
                              use_accept, da);
    };
    if (plan.wide_lds) {
        // more than one tile of site-states: the tasks' four sums travel through a per-lane block [item][task][4]
        double *tile_sums = nullptr;
        if (plan.mfma_tile && plan.wide_nss < ((2 * n1_max + 3) & ~3)) {
            if ((rc = ln.d_recip_sums.reserve((size_t)n_items * e->n_rtasks * 4 * sizeof(double)))) return rc;
            tile_sums = (double *)ln.d_recip_sums.p;
        }
        with_pass([&](auto COMMIT, auto BOTH) {
            with_bools([&](auto MFMA, auto TILED) {
                hipExtLaunchKernelGGL((recip_rows_wide_kernel<decltype(COMMIT)::value, decltype(BOTH)::value, decltype(MFMA)::value, decltype(TILED)::value>),
                                      dim3(n_items), dim3(kBlock), plan.wide_lds, ln.stream, a, b, 0, e->tp, e->bx, e->d_pos, e->d_nmol, e->d_res_q,
                                      e->d_trj, e->d_tw, e->d_rrows, e->d_row_first, e->n_rrows, plan.wide_rpt, plan.wide_nss, Ab, d_items, d_cand,
                                      site_stride, d_u, d_u_old, tile_sums, e->n_rtasks);
            }, plan.mfma_tile > 0, tile_sums != nullptr);
        });
    } else if (decide) {
        rows(recip_rows_kernel<false, true, true>, 0, *decide);
    } else if (store_alt) {
        rows(recip_rows_kernel<false, true, false, 1>, 0, no_decide);
    } else if (by_rows) {
        with_pass([&](auto COMMIT, auto BOTH) { rows(recip_rows_kernel<decltype(COMMIT)::value, decltype(BOTH)::value>, accept ? 1 : 0, no_decide); });
    } else {
        with_pass([&](auto COMMIT, auto BOTH) {
            hipExtLaunchKernelGGL((recip_kernel<decltype(COMMIT)::value, decltype(BOTH)::value>), dim3(n_items), dim3(kBlock), plan.lds, ln.stream, a,
                                  b, 0, e->tp, e->bx, e->d_pos, e->d_nmol, e->d_res_q, e->d_kpack, e->d_kslot, e->d_kw, Ab, d_items, d_cand,
                                  site_stride, plan.tile, d_u, d_u_old);
        });
    }
    rc = prof_end(e, ln, slot, a, b);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// The commit of the lane's last trial by switching A(k) buffers (commit_switch_kernel): d_items are the trial's candidates,
// `accept` marks the committed ones; the trial stored their A + delta (launch_recip's store_alt).  Timed as the commit.
int launch_commit_switch(mgpu_engine *e, Lane &ln, const RecipItem *d_items, int n_items, int site_stride, const AcceptBits &accept) {
    hipEvent_t a = nullptr, b = nullptr;
    int rc = prof_begin(e, ln, MGPU_KERNEL_COMMIT, &a, &b);
    if (rc) return rc;
    hipExtLaunchKernelGGL(commit_switch_kernel, dim3((n_items + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, ln.stream, a, b, 0,
                          e->tp, e->d_pos, e->d_nmol, d_items, n_items, (const double *)ln.d_sites.p, site_stride, accept, e->d_acur);
    rc = prof_end(e, ln, MGPU_KERNEL_COMMIT, a, b);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// S(k) of one replica into dst[Nk]
int launch_sfactor(mgpu_engine *e, int replica, double2 *dst) {
    const int ncap = e->tp.n_cap_atoms;
    hipEvent_t a = nullptr, b = nullptr;
    int rc = prof_begin(e, e->lanes[0], MGPU_KERNEL_SFACTOR, &a, &b);
    if (rc) return rc;
    hipLaunchKernelGGL(phase_table_kernel, dim3((ncap + 255) / 256), dim3(256), 0, e->stream, e->tp, e->bx, e->d_pos,
                       e->d_nmol, e->d_atom_res, e->d_atom_mol, replica, e->d_phase_tab);
    hipExtLaunchKernelGGL(sfactor_kernel, dim3(e->nk), dim3(kBlock), 0, e->stream, a, b, 0, e->tp, e->bx, e->d_nmol,
                          e->d_atom_res, e->d_atom_mol, e->d_atom_q, e->d_kpack, e->d_kslot, replica, e->d_phase_tab, dst);
    rc = prof_end(e, e->lanes[0], MGPU_KERNEL_SFACTOR, a, b);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

// ComputeIntraResidueRealCoulombEnergySingleMol for items already on the device: one thread per molecule of up to
// kIntraThreadMax sites, one wave per larger one (each kernel skips the other's items; a kernel none of whose items can be
// its own is not launched)
int launch_intra(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, const double *d_sites, int site_stride, double *d_out) {
    if (n_items <= 0) return MGPU_OK;
    bool small = false, large = false;
    for (int t = 0; t < e->tp.n_res; ++t) {
        if (e->tp.n1[t] > kIntraThreadMax) large = true;
        else small = true;
    }
    if (small)
        hipLaunchKernelGGL(intra_kernel, dim3((n_items + 63) / 64), dim3(64), 0, ln.stream, e->tp, e->bx, e->d_pos, e->d_res_q, d_items,
                           n_items, d_sites, site_stride, d_out);
    if (large)
        hipLaunchKernelGGL(intra_wave_kernel, dim3(n_items), dim3(64), 0, ln.stream, e->tp, e->bx, e->d_pos, e->d_res_q, d_items,
                           n_items, d_sites, site_stride, d_out);
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

}  // namespace mgpu
