// Batched candidates and the asynchronous submission lanes (include/maniac_gpu.h): trial submit / wait / commit, device-built
// and device-decided trials, the host team that runs their per-candidate loops.
#include "mgpu_engine.h"

extern "C" {

// The frozen residue type whose framework batched trials sweep with pair_frozen_kernel right now, -1 for none: the flat
// kernels in use in an orthorhombic box, exactly one frozen type, identical in every replica and holding a molecule
// (trial_submit_impl dispatches by it, mgpu_pair_layout reports it).
static int frozen_batch_type(const mgpu_engine *e) {
    if (!e->pair_flat || !e->frozen_batch || e->bx.triclinic) return -1;
    int nf = 0, t_frozen = -1;
    for (int tt = 0; tt < e->tp.n_res; ++tt)
        if (e->frozen[tt]) { ++nf; t_frozen = tt; }
    if (nf != 1 || e->frozen_diff[t_frozen] != 0 || e->h_nmol[t_frozen] < 1) return -1;
    return t_frozen;
}

// ---- batched candidates ----------------------------------------------------------------------

// The items of mgpu_pair_energy_candidates / mgpu_intra_energy_candidates: candidate c is the resident molecule m[c] or row c
// of `sites`.  `who` heads the null-sites error.
static int candidate_pair_items(const mgpu_engine *e, int n, const int *replica, const int *t, const int *m, const int *use_resident,
                                const double *sites, int site_stride, const char *who, std::vector<PairItem> &items, bool &any_sites) {
    items.resize(n);
    any_sites = false;
    for (int c = 0; c < n; ++c) {
        const bool res = use_resident && use_resident[c];
        if (int rc = check_candidate(e, c, replica[c], t[c], m[c], res)) return rc;
        if (!res) {
            any_sites = true;
            if (e->tp.n1[t[c]] > site_stride) return set_error(MGPU_ERR_INVALID_ARG, "site_stride smaller than atoms_in_res");
        }
        items[c] = PairItem{replica[c], t[c], m[c], res ? -1 : c, 0};
    }
    if (any_sites && !sites) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": sites is null");
    return MGPU_OK;
}

int mgpu_pair_energy_candidates(mgpu_engine *e, int n, const int *replica, const int *t, const int *m,
                                const int *use_resident, const double *sites, int site_stride, double *e_nc,
                                double *e_c) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !e_nc || !e_c) return set_error(MGPU_ERR_INVALID_ARG, "pair_energy_candidates: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    std::vector<PairItem> items;
    bool any_sites;
    if ((rc = candidate_pair_items(e, n, replica, t, m, use_resident, sites, site_stride, "pair_energy_candidates", items, any_sites))) return rc;
    if ((rc = e->d_items.reserve(n * sizeof(PairItem)))) return rc;
    if ((rc = e->d_out.reserve((size_t)2 * n * sizeof(double)))) return rc;
    if ((rc = e->h_out.reserve((size_t)2 * n * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items.p, items.data(), n * sizeof(PairItem), hipMemcpyHostToDevice, e->stream));
    if (any_sites && (rc = upload_sites(e, sites, n, site_stride, t))) return rc;
    double *d_lj = (double *)e->d_out.p, *d_c = d_lj + n;
    const int nsplit = e->pair_nsplit;
    bool fast = true;
    for (int c = 0; c < n && fast; ++c) {
        fast = replica_in_range(e, replica[c]);
        if (fast && !(use_resident && use_resident[c]))
            fast = sites_in_range(e, sites + (size_t)c * site_stride * 3, e->tp.n1[t[c]]);
    }
    if ((rc = launch_pair(e, e->lanes[0], (const PairItem *)e->d_items.p, n, common_site_count(e, items), site_stride, nsplit, d_lj, d_c,
                          false, nullptr, false, fast))) return rc;
    HIP_TRY(hipMemcpyAsync(e->h_out.p, e->d_out.p, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if ((rc = sync_stream(e))) return rc;
    std::memcpy(e_nc, e->h_out.p, n * sizeof(double));
    std::memcpy(e_c, (double *)e->h_out.p + n, n * sizeof(double));
    return MGPU_OK;
}

int mgpu_recip_energy_candidates(mgpu_engine *e, int n, const int *replica, const int *t, const int *m, const int *kind,
                                 const double *sites, int site_stride, double *u) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !kind || !u) return set_error(MGPU_ERR_INVALID_ARG, "recip_energy_candidates: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    std::vector<RecipItem> items(n);
    bool any_sites = false;
    for (int c = 0; c < n; ++c) {
        if (kind[c] < MGPU_MOVE || kind[c] > MGPU_NONE) return set_error(MGPU_ERR_INVALID_ARG, "unknown candidate kind");
        const bool need_old = (kind[c] == MGPU_MOVE || kind[c] == MGPU_DELETION);
        const bool need_new = (kind[c] == MGPU_MOVE || kind[c] == MGPU_CREATION);
        if ((rc = check_candidate(e, c, replica[c], t[c], m[c], need_old))) return rc;
        if (need_new) {
            any_sites = true;
            if (e->tp.n1[t[c]] > site_stride) return set_error(MGPU_ERR_INVALID_ARG, "site_stride smaller than atoms_in_res");
        }
        items[c] = RecipItem{replica[c], t[c], m[c], kind[c], need_new ? c : -1, 0};
    }
    if (any_sites && !sites) return set_error(MGPU_ERR_INVALID_ARG, "recip_energy_candidates: sites is null");
    // one launch per form of the candidates' own types (recip_groups): results in group order, order[slot] = candidate
    std::vector<RecipGroup> groups;
    std::vector<int> order;
    recip_groups(e, items.data(), n, groups, order);
    if (!order.empty()) {
        std::vector<RecipItem> by_form(n);
        for (int s = 0; s < n; ++s) by_form[s] = items[order[s]];
        items.swap(by_form);
    }
    if ((rc = e->d_items2.reserve(n * sizeof(RecipItem)))) return rc;
    if ((rc = e->d_out.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = e->h_out.reserve((size_t)n * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items2.p, items.data(), n * sizeof(RecipItem), hipMemcpyHostToDevice, e->stream));
    if (any_sites && (rc = upload_sites(e, sites, n, site_stride, t))) return rc;
    for (const RecipGroup &g : groups)
        if ((rc = launch_recip(e, e->lanes[0], (const RecipItem *)e->d_items2.p + g.first, g.n, g.n1_max, site_stride, false, e->d_A,
                               (double *)e->d_out.p + g.first)))
            return rc;
    HIP_TRY(hipMemcpyAsync(e->h_out.p, e->d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if ((rc = sync_stream(e))) return rc;
    if (order.empty()) std::memcpy(u, e->h_out.p, n * sizeof(double));
    else for (int s = 0; s < n; ++s) u[order[s]] = ((const double *)e->h_out.p)[s];
    return MGPU_OK;
}

int mgpu_recip_form(const mgpu_engine *e, int n1_max, int kind, int out[4]) {
    if (!e || !out) return set_error(MGPU_ERR_INVALID_ARG, "mgpu_recip_form: null argument");
    if (n1_max < 1) return set_error(MGPU_ERR_INVALID_ARG, "mgpu_recip_form: n1_max must be positive");
    if (kind != MGPU_RECIP_TRIAL && kind != MGPU_RECIP_COMMIT) return set_error(MGPU_ERR_INVALID_ARG, "mgpu_recip_form: unknown kind");
    // (a trial and a commit take the same form: launch_recip decides by n1_max alone, so that they share the sum order)
    const RecipPlan p = recip_plan(e, n1_max, true);
    if (p.lds > kLdsDefaultMax) return set_error(MGPU_ERR_CAPACITY, "mgpu_recip_form: kmax too large for the LDS phase tables");
    out[0] = p.form;
    out[2] = 0;
    out[3] = 1;
    switch (p.form) {
        case MGPU_RECIP_FORM_ROWS: out[1] = 2 * n1_max; out[2] = e->n_rrows; break;
        case MGPU_RECIP_FORM_WIDE_VECTOR: out[1] = 2 * n1_max; out[2] = p.wide_rpt; break;
        case MGPU_RECIP_FORM_PER_K: out[1] = 2 * p.tile; out[3] = (n1_max + p.tile - 1) / p.tile; break;
        default: out[1] = p.mfma_tile; out[3] = (((2 * n1_max + 3) & ~3) + p.mfma_tile - 1) / p.mfma_tile; break;
    }
    return MGPU_OK;
}

int mgpu_pair_layout(const mgpu_engine *e, int out[MGPU_PAIR_LAYOUT_LEN]) {
    if (!e || !out) return set_error(MGPU_ERR_INVALID_ARG, "mgpu_pair_layout: null argument");
    out[0] = e->pair_flat ? 1 : 0;
    out[1] = e->flat_groups;
    out[2] = e->flat_planes;
    out[3] = frozen_batch_type(e);
    for (int t = 0; t < kMaxRes; ++t) out[4 + t] = t < e->tp.n_res ? e->tp.site_major[t] : -1;
    return MGPU_OK;
}

int mgpu_self_energy(const mgpu_engine *e, int t, double *e_self) {
    if (!e || !e_self) return set_error(MGPU_ERR_INVALID_ARG, "mgpu_self_energy: null argument");
    if (t < 0 || t >= e->tp.n_res) return set_error(MGPU_ERR_INVALID_ARG, "residue type out of range");
    *e_self = self_energy_host(e, t);
    return MGPU_OK;
}

int mgpu_intra_energy_candidates(mgpu_engine *e, int n, const int *replica, const int *t, const int *m,
                                 const int *use_resident, const double *sites, int site_stride, double *u) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !u) return set_error(MGPU_ERR_INVALID_ARG, "intra_energy_candidates: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    std::vector<PairItem> items;
    bool any_sites;
    if ((rc = candidate_pair_items(e, n, replica, t, m, use_resident, sites, site_stride, "intra_energy_candidates", items, any_sites))) return rc;
    if ((rc = e->d_items.reserve(n * sizeof(PairItem)))) return rc;
    if ((rc = e->d_out.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = e->h_out.reserve((size_t)n * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_items.p, items.data(), n * sizeof(PairItem), hipMemcpyHostToDevice, e->stream));
    if (any_sites && (rc = upload_sites(e, sites, n, site_stride, t))) return rc;
    if ((rc = launch_intra(e, e->lanes[0], (const PairItem *)e->d_items.p, n, (const double *)e->d_sites.p, site_stride, (double *)e->d_out.p)))
        return rc;
    HIP_TRY(hipMemcpyAsync(e->h_out.p, e->d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if ((rc = sync_stream(e))) return rc;
    std::memcpy(u, e->h_out.p, n * sizeof(double));
    return MGPU_OK;
}

// Queue one trial per candidate on a lane: inputs are staged through pinned host memory, so the call
// returns as soon as the copies and the kernels are enqueued.  kind == nullptr: all MGPU_MOVE.
// Per candidate (ComputeOldEnergy / ComputeNewEnergy, monte_carlo_utils.f90:275-395):
//   MOVE      pair(resident) | pair(sites)          recip(A) | recip(A + new - old)
//   CREATION  --             | pair(sites), intra   recip(A) | recip(A + new)         (m ignored)
//   DELETION  pair(resident), intra | --            recip(A) | recip(A - old)
// One pass over k per candidate yields both reciprocal energies.  The staging block and the result block: TrialStaging,
// TrialResult (mgpu_internal.h); the lane remembers where each candidate's pair entries are.
// build != nullptr: the candidate rows are built on the device (trial_build_kernel) from the molecule frames, the move
// codes (1 translation, 2 rotation, 3 creation, 4 deletion) and five uniform numbers per candidate; `sites` is null and
// site_stride is ignored (a row is [sites (n1_max) | com | offsets (n1_max)])
struct TrialBuild {
    const int *move;
    const double *u;              // [n][5]
    double t_step, r_step;
};
// decide != nullptr: the acceptance test runs on the device behind the k sweep and accepted candidates are committed there
// (DecideItem, mgpu_kernels_recip.h); accept_u[n] = the test's uniform numbers, accept_pref[n] = its prefactors
struct TrialDecide {
    const double *u, *pref;
    double temperature;
};
// the accepted share of a lane's commits above which its trials store A + delta for a commit by switching (Lane::accept_share)
constexpr double kSwitchMinShare = 0.5;

// A batched trial between the stages of trial_submit_impl.  Candidates are grouped by residue type (a class): every type
// gets its own pair-sweep launches with the register-site kernels of its size (a mixture of a 3-site and a 2-site species
// used to fall to the generic NS = 0 sweep for the whole launch), and which kernels a type's candidates take never depends
// on what else shares the launch.  Within a type, trial moves of molecules with a few sites are swept old + new together
// (a fused segment: two entries per item); insertions, deletions and everything else are single-state items.
struct Seg { int n1, fused, first_item, n_items, first_entry, n_entries, type, nsplit, first_partial, batched; };
struct TrialPlan {
    int n = 0, n_cls = 0;
    int cls_n1[kMaxRes], cls_moves[kMaxRes], cls_single[kMaxRes], cls_type[kMaxRes];
    int seg_fused[kMaxRes], seg_single[kMaxRes];        // per class: index of its fused / single segment (-1: none)
    std::vector<Seg> segs;
    int n_pair = 0, n_partials = 0, n_intra = 0, n1_max = 1;
    bool fast = true;                 // all replicas of this trial within the fast fold's range
    // Framework boxes: one frozen residue type, identical in every replica, flat kernels in use, an active residue type of
    // <= 5 sites -> the type's segments are `batched`: their items go to pair_frozen_kernel (candidates in the lanes; framework
    // atoms as scalars, then the replica's few other atoms per lane); their sums arrive as ONE extra record per entry behind
    // the other results
    int t_frozen = -1, n_chunks_f = 0;
    size_t scratch_records = 0;       // chunk partials of those sweeps
    TrialStaging in{};                // the two blocks (mgpu_internal.h)
    TrialResult out{};
};

// Stage 1: the classes and their segments, with every segment's place among the items, entries and partials; the result block.
static int trial_plan(const mgpu_engine *e, int n, const int *t, const int *kind, bool decide, TrialPlan &pl) {
    for (int c = 0; c < n; ++c) {
        const int k = kind ? kind[c] : MGPU_MOVE;
        if (k < MGPU_MOVE || k > MGPU_DELETION) return set_error(MGPU_ERR_INVALID_ARG, "trial_submit: unknown candidate kind");
        if (t[c] < 0 || t[c] >= e->tp.n_res) return set_error(MGPU_ERR_INVALID_ARG, "trial_submit: residue type out of range");
        const int n1 = e->tp.n1[t[c]];
        int ci = 0;
        while (ci < pl.n_cls && pl.cls_type[ci] != t[c]) ++ci;
        if (ci == pl.n_cls) { pl.cls_n1[ci] = n1; pl.cls_moves[ci] = 0; pl.cls_single[ci] = 0; pl.cls_type[ci] = t[c]; ++pl.n_cls; }   // <= n_res classes
        // (triclinic boxes: two single-state items -- the image search's registers leave no room for 2 NS sites without spills;
        //  measured round 5, 10 125-atom box, 1024 moves: fused 267-391 us, two single-state sweeps 239 us)
        const bool fz = k == MGPU_MOVE && n1 <= kMaxFusedSites && !e->bx.triclinic;
        if (fz) pl.cls_moves[ci] += 1;
        else pl.cls_single[ci] += (k == MGPU_MOVE) ? 2 : 1;
    }
    pl.t_frozen = frozen_batch_type(e);
    const int n_atoms_f = pl.t_frozen >= 0 ? e->h_nmol[pl.t_frozen] * e->tp.n1[pl.t_frozen] : 0;
    pl.n_chunks_f = pl.t_frozen >= 0 ? (n_atoms_f + frozen_chunk_atoms(e, n_atoms_f) - 1) / frozen_chunk_atoms(e, n_atoms_f) : 0;
    int n_items_total = 0;
    for (int ci = 0; ci < pl.n_cls; ++ci) {
        const int n1 = pl.cls_n1[ci], ty = pl.cls_type[ci];
        const int batched = pl.t_frozen >= 0 && ty != pl.t_frozen && n1 <= kMaxFusedSitesWide;
        const int ns_seg = batched ? 0 : e->pair_nsplit;      // batched: the extra record is all
        auto add_seg = [&](int fused, int n_items, int &seg_of_class) {
            seg_of_class = n_items ? (int)pl.segs.size() : -1;
            if (!n_items) return;
            const int n_entries = fused ? 2 * n_items : n_items;
            pl.segs.push_back(Seg{n1, fused, n_items_total, n_items, pl.n_pair, n_entries, ty, ns_seg, pl.n_partials, batched});
            n_items_total += n_items;
            pl.n_pair += n_entries;
            pl.n_partials += n_entries * ns_seg;
            if (batched) pl.scratch_records += (size_t)n_entries * pl.n_chunks_f;
        };
        add_seg(1, pl.cls_moves[ci], pl.seg_fused[ci]);
        add_seg(0, pl.cls_single[ci], pl.seg_single[ci]);
    }
    pl.out = trial_result(n, pl.n_partials, pl.n_pair, pl.scratch_records != 0, decide);
    return MGPU_OK;
}

// Stage 2: validate every candidate and write its pair, k and intra items into the staging block, the lane's per-candidate
// rows beside them.  Two passes over the candidates, each cut into ranges run side by side (for_parts): the first validates
// a candidate, fills what belongs to it alone and counts the items it will add to its class's segments; the second, knowing
// every range's first item in every segment, writes the items -- in candidate order within a segment, as one loop would.
static int trial_fill(mgpu_engine *e, Lane &ln, TrialPlan &pl, const int *replica, const int *t, const int *m, const int *kind,
                      const double *sites, const TrialBuild *build, const TrialDecide *decide) {
    const int n = pl.n, n_cls = pl.n_cls, site_stride = pl.in.row_sites, frame_at = pl.in.frame_at;
    PairItem *pit = (PairItem *)((char *)ln.h_in.p + pl.in.pair_items), *iit = (PairItem *)((char *)ln.h_in.p + pl.in.intra_items);
    RecipItem *rit = (RecipItem *)((char *)ln.h_in.p + pl.in.k_items);
    ln.pair_old.assign(n, -1);
    ln.pair_new.assign(n, -1);
    ln.intra_idx.assign(n, -1);
    ln.kinds.assign(n, MGPU_MOVE);
    ln.self_of.assign(n, 0.0);
    ln.ent_off.assign(pl.n_pair, 0);
    ln.ent_stride.assign(pl.n_pair, 2);
    ln.ent_ns.assign(pl.n_pair, 1);
    ln.cand_ok.assign(n, 1);          // per candidate: would committing it keep its replica within the fast fold's range
    auto put_item = [&](const Seg &sg, int i, const PairItem &it) {     // item i of the segment; returns its first entry
        pit[sg.first_item + i] = it;
        const int e0 = sg.first_entry + (sg.fused ? 2 * i : i);
        // partial records (double2) of the segment start at first_partial; [split][state] for fused items
        if (sg.fused) {
            ln.ent_off[e0] = 2 * (sg.first_partial + 2 * i * sg.nsplit);
            ln.ent_off[e0 + 1] = ln.ent_off[e0] + 2;
            ln.ent_stride[e0] = ln.ent_stride[e0 + 1] = 4;
            ln.ent_ns[e0] = ln.ent_ns[e0 + 1] = sg.nsplit;
        } else {
            ln.ent_off[e0] = 2 * (sg.first_partial + i * sg.nsplit);
            ln.ent_ns[e0] = sg.nsplit;
        }
        return e0;
    };
    struct Part {
        int n1_max = 1, n_intra = 0;
        bool fast = true;
        int n_fused[kMaxRes], n_single[kMaxRes];
        int at_fused[kMaxRes], at_single[kMaxRes], at_intra = 0;
    };
    const int parts = host_parts(e, n);
    Part part_of[kMaxHostParts];
    PartError errs[kMaxHostParts];
    auto class_of = [&](int ty) { int ci = 0; while (pl.cls_type[ci] != ty) ++ci; return ci; };
    // candidate c's pair and intra items at the places the running indices say
    auto place = [&](int c, int k, int mc, int ci, int *i_f, int *i_s, int &i_intra) {
        if (k == MGPU_MOVE && pl.seg_fused[ci] >= 0) {
            const int e0 = put_item(pl.segs[pl.seg_fused[ci]], i_f[ci]++, PairItem{replica[c], t[c], mc, c, 0});
            ln.pair_old[c] = e0; ln.pair_new[c] = e0 + 1;
        } else {
            const Seg &sg = pl.segs[pl.seg_single[ci]];
            if (k != MGPU_CREATION) ln.pair_old[c] = put_item(sg, i_s[ci]++, PairItem{replica[c], t[c], mc, -1, 0});
            if (k != MGPU_DELETION) ln.pair_new[c] = put_item(sg, i_s[ci]++, PairItem{replica[c], t[c], mc, c, 0});
        }
        if (k == MGPU_CREATION) { ln.intra_idx[c] = i_intra; iit[i_intra++] = PairItem{replica[c], t[c], -1, c, 0}; }
        if (k == MGPU_DELETION) { ln.intra_idx[c] = i_intra; iit[i_intra++] = PairItem{replica[c], t[c], mc, -1, 0}; }
    };
    for_parts(parts, [&](int q) {
        Part &P = part_of[q];
        for (int ci = 0; ci < n_cls; ++ci) P.n_fused[ci] = P.n_single[ci] = 0;
        int c0, c1;
        part_range(n, parts, q, c0, c1);
        std::string why;
        for (int c = c0; c < c1; ++c) {
            const int k = kind ? kind[c] : MGPU_MOVE;
            const int mc = (k == MGPU_CREATION) ? -1 : m[c];
            if (const int r = check_candidate(e, c, replica[c], t[c], mc, k != MGPU_CREATION)) { errs[q].set(c, r, mgpu_last_error()); return; }
            const int n1 = e->tp.n1[t[c]];
            if (n1 > site_stride) { errs[q].set(c, MGPU_ERR_INVALID_ARG, "site_stride smaller than atoms_in_res"); return; }
            P.n1_max = std::max(P.n1_max, n1);
            const int ci = class_of(t[c]);
            ln.kinds[c] = k;
            P.fast = P.fast && replica_in_range(e, replica[c]);
            const size_t idx = (size_t)replica[c] * e->tp.n_res + t[c];
            if (build) {
                if (const int r = admit_built(e, idx, k, build->move[c], kAdmitAll, "move_trial_submit", "candidate", c, why, ln.cand_ok[c], P.fast)) {
                    errs[q].set(c, r, why);
                    return;
                }
            } else if (k != MGPU_DELETION) {
                ln.cand_ok[c] = sites_in_range(e, sites + (size_t)c * site_stride * 3, n1) ? 1 : 0;
                P.fast = P.fast && ln.cand_ok[c];          // the candidate's own sites are swept in this launch
            }
            if (k != MGPU_MOVE) ln.self_of[c] = e->self_of_type[t[c]];
            if (decide) {
                if (k == MGPU_CREATION && e->h_nmol[idx] >= e->tp.cap[t[c]]) {
                    errs[q].set(c, MGPU_ERR_CAPACITY, "trial_decide_submit: residue type is at mol_capacity");
                    return;
                }
                if (!build && k != MGPU_DELETION && e->d_com && e->frames_ok[idx]) {
                    errs[q].set(c, MGPU_ERR_STATE, "trial_decide_submit: this replica holds molecule frames: submit device-built trials");
                    return;
                }
            }
            rit[c] = RecipItem{replica[c], t[c], mc, k, k == MGPU_DELETION ? -1 : c, 0, frame_at};   // one k sweep: old and new
            if (parts == 1) {            // one range: its counters ARE the items' places, no second pass
                place(c, k, mc, ci, P.n_fused, P.n_single, P.n_intra);
                continue;
            }
            if (k == MGPU_MOVE && pl.seg_fused[ci] >= 0) P.n_fused[ci] += 1;
            else P.n_single[ci] += (k != MGPU_CREATION) + (k != MGPU_DELETION);
            if (k != MGPU_MOVE) P.n_intra += 1;
        }
    });
    if (int rc = report_first(errs, parts)) return rc;
    int run_f[kMaxRes] = {0}, run_s[kMaxRes] = {0};
    for (int q = 0; q < parts; ++q) {
        Part &P = part_of[q];
        pl.n1_max = std::max(pl.n1_max, P.n1_max);
        pl.fast = pl.fast && P.fast;
        P.at_intra = pl.n_intra;
        pl.n_intra += P.n_intra;
        for (int ci = 0; ci < n_cls; ++ci) {
            P.at_fused[ci] = run_f[ci]; run_f[ci] += P.n_fused[ci];
            P.at_single[ci] = run_s[ci]; run_s[ci] += P.n_single[ci];
        }
    }
    if (parts > 1)
        for_parts(parts, [&](int q) {
            const Part &P = part_of[q];
            int i_f[kMaxRes], i_s[kMaxRes], i_intra = P.at_intra;
            for (int ci = 0; ci < n_cls; ++ci) { i_f[ci] = P.at_fused[ci]; i_s[ci] = P.at_single[ci]; }
            int c0, c1;
            part_range(n, parts, q, c0, c1);
            for (int c = c0; c < c1; ++c) {
                const int k = ln.kinds[c];
                place(c, k, (k == MGPU_CREATION) ? -1 : m[c], class_of(t[c]), i_f, i_s, i_intra);
            }
        });
    return MGPU_OK;
}

// the deciding form's records: where the device finds each candidate's pair entries, intra result and constants
static void trial_decide_items(Lane &ln, const TrialPlan &pl, const TrialDecide &decide) {
    DecideItem *dit = (DecideItem *)((char *)ln.h_in.p + pl.in.decide_items);
    for (int c = 0; c < pl.n; ++c) {
        DecideItem d{0, 2, -1, -1, 0, 2, -1, -1, ln.intra_idx[c], ln.kinds[c], ln.self_of[c], decide.pref[c], decide.u[c]};
        if (const int i = ln.pair_old[c]; i >= 0) {
            d.old_off = ln.ent_off[i]; d.old_stride = ln.ent_stride[i]; d.old_ns = ln.ent_ns[i];
            d.old_extra = ln.ent_extra[i] ? (int)(pl.out.extra + 2 * (size_t)i) : -1;
        }
        if (const int i = ln.pair_new[c]; i >= 0) {
            d.new_off = ln.ent_off[i]; d.new_stride = ln.ent_stride[i]; d.new_ns = ln.ent_ns[i];
            d.new_extra = ln.ent_extra[i] ? (int)(pl.out.extra + 2 * (size_t)i) : -1;
        }
        dit[c] = d;
    }
}

// Stage 3: finish the staging block (site rows or the build's inputs, decide items), reserve the device blocks, and send the
// staging block to the device -- one H2D copy; rows built on the device are written there by trial_build_kernel.
static int trial_stage(mgpu_engine *e, Lane &ln, const TrialPlan &pl, const int *t, const double *sites, const TrialBuild *build,
                       const TrialDecide *decide) {
    const int n = pl.n;
    char *h_in = (char *)ln.h_in.p;
    if (build) {
        std::memcpy(h_in + pl.in.moves, build->move, (size_t)n * sizeof(int));
        std::memcpy(h_in + pl.in.uniforms, build->u, (size_t)5 * n * sizeof(double));
    } else {
        if (sites != ln.h_in.p) std::memcpy(h_in, sites, pl.in.pair_items);    // rows built in place (mgpu_lane_site_buffer): no copy
        if (any_frozen(e, n, t)) permute_frozen_rows(e, (double *)h_in, n, pl.in.row_sites, t);
    }
    ln.ent_extra.assign(pl.n_pair, 0);
    for (const Seg &sg : pl.segs)
        if (sg.batched) std::fill_n(ln.ent_extra.begin() + sg.first_entry, sg.n_entries, 1);
    int rc;
    if (decide) {
        if (!recip_by_rows(e, pl.n1_max)) return set_error(MGPU_ERR_STATE, "trial_decide_submit: needs the row-form k sweep");
        trial_decide_items(ln, pl, *decide);
    }
    if (pl.scratch_records && (rc = ln.d_scratch.reserve(pl.scratch_records * sizeof(double2)))) return rc;
    if ((rc = ln.d_sites.reserve(pl.in.total))) return rc;
    if ((rc = ln.d_out.reserve(pl.out.total * sizeof(double)))) return rc;
    if ((rc = ln.h_out.reserve(pl.out.total * sizeof(double)))) return rc;
    char *d_in = (char *)ln.d_sites.p;
    if (build) {
        // the rows are written by the device: only [items | move codes | uniforms | decide items] travel
        HIP_TRY(hipMemcpyAsync(d_in + pl.in.pair_items, h_in + pl.in.pair_items, pl.in.total - pl.in.pair_items, hipMemcpyHostToDevice, ln.stream));
        // (a triclinic cell: the instance with trial_com_triclinic's centre; the entry points refuse one without the switch)
        const auto build_kernel = e->bx.triclinic ? trial_build_kernel<true> : trial_build_kernel<false>;
        hipLaunchKernelGGL(build_kernel, dim3((n + 127) / 128), dim3(128), 0, ln.stream, e->tp, e->bx, (const RecipItem *)(d_in + pl.in.k_items),
                           (const int *)(d_in + pl.in.moves), (const double *)(d_in + pl.in.uniforms), build->t_step, build->r_step,
                           (double *)d_in, pl.in.row_sites, pl.in.frame_at, n, pl.in.pick_at);
        HIP_TRY(hipGetLastError());
    } else {
        // (only the intra items in use travel)
        HIP_TRY(hipMemcpyAsync(d_in, h_in, pl.in.intra_items + (size_t)pl.n_intra * sizeof(PairItem), hipMemcpyHostToDevice, ln.stream));
        if (decide)
            HIP_TRY(hipMemcpyAsync(d_in + pl.in.decide_items, h_in + pl.in.decide_items, pl.in.total - pl.in.decide_items, hipMemcpyHostToDevice, ln.stream));
    }
    return MGPU_OK;
}

// Stage 4: the sweeps.  Kernel order: pair sweep first, k sweep second (the order the stand-alone commit of the other lanes
// overlaps best with; k sweep first was measured 10 % slower there), then intra; the deciding k sweep comes last: its
// workgroups decide and commit (everything else of the trial has read the old state).
static int trial_launch(mgpu_engine *e, Lane &ln, const TrialPlan &pl, const int *replica, const TrialDecide *decide) {
    const int n = pl.n, site_stride = pl.in.row_sites;
    int rc;
    const char *d_in = (const char *)ln.d_sites.p;
    const PairItem *d_pit = (const PairItem *)(d_in + pl.in.pair_items), *d_iit = (const PairItem *)(d_in + pl.in.intra_items);
    const RecipItem *d_rit = (const RecipItem *)(d_in + pl.in.k_items), *rit = (const RecipItem *)((char *)ln.h_in.p + pl.in.k_items);
    double *d_out = (double *)ln.d_out.p;
    double2 *d_part = (double2 *)(d_out + pl.out.partials);
    double *d_uo = d_out + pl.out.u_old, *d_un = d_out + pl.out.u_new, *d_intra = d_out + pl.out.intra;
    size_t scratch_at = 0;
    for (const Seg &sg : pl.segs) {
        if (!sg.batched && (rc = launch_pair(e, ln, d_pit + sg.first_item, sg.n_items, sg.n1, site_stride, sg.nsplit, nullptr, nullptr, false,
                                     d_part + sg.first_partial, sg.fused != 0, pl.fast)))
            return rc;
        if (sg.batched) {
            if ((rc = launch_frozen(e, ln, d_pit + sg.first_item, sg.n_items, sg.n1, site_stride, sg.fused != 0, pl.fast, pl.t_frozen,
                                    (double2 *)ln.d_scratch.p + scratch_at, (double2 *)(d_out + pl.out.extra) + sg.first_entry)))
                return rc;
            scratch_at += (size_t)sg.n_entries * pl.n_chunks_f;
        }
    }
    ln.recip_slot.clear();
    if (!decide) {
        // one k sweep per form of the candidates' own types (recip_groups; a trial of one type, or of row-form types only,
        // is one launch over d_rit as it stands): a candidate's energies do not depend on what shares its trial
        recip_groups(e, rit, n, ln.recip_groups, ln.recip_order);
        const RecipItem *d_rit_k = d_rit;
        if (!ln.recip_order.empty()) {
            const size_t rit_bytes = (size_t)n * sizeof(RecipItem);
            if ((rc = ln.h_recip_items.reserve(rit_bytes)) || (rc = ln.d_recip_items.reserve(rit_bytes))) return rc;
            RecipItem *h = (RecipItem *)ln.h_recip_items.p;
            ln.recip_slot.resize(n);
            for (int s = 0; s < n; ++s) { h[s] = rit[ln.recip_order[s]]; ln.recip_slot[ln.recip_order[s]] = s; }
            HIP_TRY(hipMemcpyAsync(ln.d_recip_items.p, h, rit_bytes, hipMemcpyHostToDevice, ln.stream));
            d_rit_k = (const RecipItem *)ln.d_recip_items.p;
        }
        // A trial whose commit can switch A(k) buffers (commit_from_trial): its k sweep also stores every candidate's A + delta
        // into the replica's other buffer.  One row-form launch (the commit by accept mask's form, whose sums it shares), one
        // candidate per replica (their stores would collide), molecules of at most 64 sites (commit_switch_kernel), and a
        // lane whose last commit accepted at least kSwitchMinShare of its candidates.
        bool alt = !e->commit_pass && ln.accept_share >= kSwitchMinShare && ln.recip_groups.size() == 1 && recip_by_rows(e, pl.n1_max) && pl.n1_max <= 64 && n <= 32 * kAcceptWords;
        alt = alt && one_record_per_replica(ln, e->n_replicas, replica, n);
        if (alt && (rc = alt_reserve(e))) return rc;
        if (alt) {
            ln.trial_stamp = ++e->trial_stamps;
            for (int c = 0; c < n; ++c) __atomic_store_n(&e->alt_owner[replica[c]], ln.trial_stamp, __ATOMIC_RELAXED);
        }
        for (const RecipGroup &g : ln.recip_groups)
            if ((rc = launch_recip(e, ln, d_rit_k + g.first, g.n, g.n1_max, site_stride, false, e->d_A, d_un + g.first, d_uo + g.first,
                                   nullptr, nullptr, nullptr, alt)))
                return rc;
        ln.trial_alt = alt;
    }
    if (pl.n_intra && (rc = launch_intra(e, ln, d_iit, pl.n_intra, (const double *)d_in, site_stride, d_intra))) return rc;
    if (decide) {
        const DecideArgs da{(const DecideItem *)(d_in + pl.in.decide_items), d_out, d_intra, (int *)(d_out + pl.out.flags), decide->temperature};
        if ((rc = launch_recip(e, ln, d_rit, n, pl.n1_max, site_stride, false, e->d_A, d_un, d_uo, nullptr, nullptr, &da))) return rc;
    }
    return MGPU_OK;
}

// Stage 5: the copy-out, and everything the lane remembers of the trial in flight.
static int trial_record(mgpu_engine *e, Lane &ln, const TrialPlan &pl, const int *replica, bool built, bool decided) {
    const int n = pl.n;
    ln.result = pl.out;
    if (decided) {
        for (int c = 0; c < n; ++c) alt_forget(e, replica[c]);      // (its accepted candidates are committed in place)
        ln.decided_n = n;
        ln.decided_wait_n = n;
    }
    HIP_TRY(hipMemcpyAsync(ln.h_out.p, ln.d_out.p, pl.out.total * sizeof(double), hipMemcpyDeviceToHost, ln.stream));
    ln.n_submitted = n;
    ln.n_pair_items = pl.n_pair;
    ln.last_trial_n = n;
    ln.last_trial_stride = pl.in.row_sites;
    ln.last_trial_built = built;
    ln.last_trial_frame = pl.in.frame_at;
    ln.d_trial_items = (const RecipItem *)((const char *)ln.d_sites.p + pl.in.k_items);
    ln.h_trial_items = (const RecipItem *)((const char *)ln.h_in.p + pl.in.k_items);
    ln.trial_n1_max = pl.n1_max;
    return MGPU_OK;
}

static int trial_submit_impl(mgpu_engine *e, Lane &ln, int n, const int *replica, const int *t, const int *m,
                             const int *kind, const double *sites, int site_stride, const TrialBuild *build = nullptr,
                             const TrialDecide *decide = nullptr) {
    if (ln.n_submitted != 0) return set_error(MGPU_ERR_STATE, "trial_submit: the lane still holds an un-waited trial");
    int rc;
    if (decide) {
        if (!(decide->temperature > 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "trial_decide_submit: temperature must be positive");
        // one candidate per replica: the workgroups commit independently
        for (int c = 0; c < n; ++c)
            if (replica[c] < 0 || replica[c] >= e->n_replicas) return set_error(MGPU_ERR_INVALID_ARG, "trial_decide_submit: replica out of range");
        if (!one_record_per_replica(ln, e->n_replicas, replica, n)) return set_error(MGPU_ERR_INVALID_ARG, "trial_decide_submit: more than one candidate for a replica");
    }
    ln.decided_wait_n = 0;
    ln.dirty = true;
    ln.last_trial_built = false;
    if (build) {      // rows of the largest molecule's size; site_stride came in as 0
        site_stride = 1;
        for (int c = 0; c < n; ++c) {
            if (t[c] < 0 || t[c] >= e->tp.n_res) return set_error(MGPU_ERR_INVALID_ARG, "trial_submit: residue type out of range");
            site_stride = std::max(site_stride, e->tp.n1[t[c]]);
        }
    }
    // from here on the rows of the lane's previous trial are gone (the staging block below may be regrown and is
    // overwritten): a failed submit must not leave them committable "from the lane's resident rows"
    ln.forget_trial();
    TrialPlan pl;
    pl.n = n;
    pl.in = trial_staging(n, site_stride, build != nullptr, e->rsv_any, decide != nullptr);
    // (up to the move codes: the rows and items every trial has)
    if (sites && sites == ln.h_in.p && pl.in.moves > ln.h_in.bytes)
        return set_error(MGPU_ERR_INVALID_ARG, "trial_submit: more candidates than the lane's site buffer was sized for");
    if (sites && sites == ln.h_in.p && pl.in.total > ln.h_in.bytes)
        return set_error(MGPU_ERR_INVALID_ARG, "trial_decide_submit: the lane's site buffer is too small for the acceptance records "
                                               "(mgpu_lane_site_buffer sizes it for them)");
    // a block lent to the caller is never regrown behind their back (they keep the pointer for the farm's lifetime)
    if (ln.h_in_lent && pl.in.total > ln.h_in.bytes)
        return set_error(MGPU_ERR_STATE, "trial_submit: this trial needs a larger staging block than the one lent out by "
                                         "mgpu_lane_site_buffer; call it again with the larger size first");
    if ((rc = ln.h_in.reserve(pl.in.total))) return rc;
    if ((rc = trial_plan(e, n, t, kind, decide != nullptr, pl))) return rc;
    if ((rc = trial_fill(e, ln, pl, replica, t, m, kind, sites, build, decide))) return rc;
    if ((rc = trial_stage(e, ln, pl, t, sites, build, decide))) return rc;
    if ((rc = trial_launch(e, ln, pl, replica, decide))) return rc;
    return trial_record(e, ln, pl, replica, build != nullptr, decide != nullptr);
}

// ncomp = 3: non_coulomb, coulomb, recip_coulomb; ncomp = 5: + ewald_self, intra_coulomb
static int trial_wait_impl(mgpu_engine *e, Lane &ln, double *old_energy, double *new_energy, int ncomp, int *accepted = nullptr) {
    const int n = ln.n_submitted;
    if (n == 0) return set_error(MGPU_ERR_STATE, "trial_wait: nothing was submitted on this lane");
    // (a drain in between -- mgpu_synchronize or any synchronous entry point -- has already folded the outcomes into the
    // engine's mirrors; the flags are still in the result block)
    if (accepted && ln.decided_wait_n != n) return set_error(MGPU_ERR_STATE, "trial_decide_wait: the lane's trial was not submitted with an acceptance test");
    ln.decided_wait_n = 0;
    ln.n_submitted = 0;
    const TrialResult at = ln.result;
    int rc = sync_lane(e, ln);
    if (rc) return rc;
    if (accepted) std::memcpy(accepted, (const char *)ln.h_out.p + at.flags_bytes(), (size_t)n * sizeof(int));
    const int np = ln.n_pair_items;
    const double *h = (const double *)ln.h_out.p;
    const double *uo = h + at.u_old, *un = h + at.u_new, *in = h + at.intra, *ex = h + at.extra;
    // the ordered sum of the split partials and the Coulomb rescale e_coulomb * EPS0_INV_eVA / KB_eVK
    // (energy_utils.f90:440), exactly as pair_finalize_kernel does them.  Partials of a fused item are laid out
    // [split][state], those of a single item [split].
    ln.h_lj.resize(np);
    ln.h_cc.resize(np);
    const int team = host_parts(e, n);       // (both loops are independent per entry / per candidate)
#pragma omp parallel for num_threads(team) schedule(static) if (team > 1)
    for (int i = 0; i < np; ++i) {
        double a = 0.0, b = 0.0;
        const double *p = h + ln.ent_off[i];
        const int stride = ln.ent_stride[i], ns = ln.ent_ns[i];
        for (int s2 = 0; s2 < ns; ++s2) { a += p[stride * s2]; b += p[stride * s2 + 1]; }
        if (ln.ent_extra[i]) { a += ex[2 * i]; b += ex[2 * i + 1]; }       // the framework part (pair_frozen_kernel), last
        ln.h_lj[i] = a;
        ln.h_cc[i] = b * kEps0InvEvA / kKbEvK;
    }
    const double *lj = ln.h_lj.data(), *cc = ln.h_cc.data();
#pragma omp parallel for num_threads(team) schedule(static) if (team > 1)
    for (int c = 0; c < n; ++c) {
        double *o = old_energy + (size_t)ncomp * c, *w = new_energy + (size_t)ncomp * c;
        for (int k = 0; k < ncomp; ++k) { o[k] = 0.0; w[k] = 0.0; }
        if (ln.pair_old[c] >= 0) { o[0] = lj[ln.pair_old[c]]; o[1] = cc[ln.pair_old[c]]; }
        if (ln.pair_new[c] >= 0) { w[0] = lj[ln.pair_new[c]]; w[1] = cc[ln.pair_new[c]]; }
        const int slot = ln.recip_slot.empty() ? c : ln.recip_slot[c];
        o[2] = uo[slot];
        w[2] = un[slot];
        if (ncomp == 5) {
            // ewald_self / intra_coulomb enter on the side where the molecule exists
            // (monte_carlo_utils.f90:298-299 creation new, :378-379 deletion old)
            if (ln.kinds[c] == MGPU_CREATION) { w[3] = ln.self_of[c]; w[4] = in[ln.intra_idx[c]]; }
            if (ln.kinds[c] == MGPU_DELETION) { o[3] = ln.self_of[c]; o[4] = in[ln.intra_idx[c]]; }
        }
    }
    return MGPU_OK;
}

// What a range of commit_collect's candidates leaves for the commit's tail
struct CommitPart {
    int n_acc = 0, at = 0;
    bool any_sites = false;
    std::vector<int> new_counts;  // (index into h_nmol, value) pairs applied after validation
    std::vector<int> range_lost;  // (replica, type) entries whose atoms leave the fast fold's range with this commit
};

// A refused commit_collect: take its stamps back (a repeat of the call must not look like a duplicate) and settle which error
// the serial loop would have reported.  Two accepted candidates of one replica in DIFFERENT ranges are noticed by whichever
// range came second in time: which candidate that is depends on the threads.  The serial loop reports the second of the pair
// in candidate order, and it stops at the first refusal of any kind: scan for a duplicate below the refusal just found.
static int commit_refused(mgpu_engine *e, Lane &ln, int n, const int *replica, const int *accept, const PartError *errs, int parts, int rc) {
    auto unmark = [&] {
        for (int c = 0; c < n; ++c)
            if (accept[c] && replica[c] >= 0 && replica[c] < e->n_replicas) ln.commit_mark[replica[c]] = -1;
    };
    unmark();
    if (parts == 1) return rc;
    int first_bad = n;
    for (int q = 0; q < parts; ++q)
        if (errs[q].c >= 0) first_bad = std::min(first_bad, errs[q].c);
    const int scan = ++ln.commit_stamp;
    int dup = -1;
    for (int c = 0; c < n && c <= first_bad && dup < 0; ++c) {
        if (!accept[c] || replica[c] < 0 || replica[c] >= e->n_replicas) continue;
        if (ln.commit_mark[replica[c]] == scan) dup = c;
        ln.commit_mark[replica[c]] = scan;
    }
    unmark();
    if (dup >= 0 && dup <= first_bad) return set_error(MGPU_ERR_INVALID_ARG, "commit: more than one accepted candidate for a replica");
    return rc;
}

// Part 1 of a commit: validate the accepted candidates and write their items, in candidate order, into `items`.  Two passes
// in ranges, as in trial_fill: count the accepted candidates of every range, then validate them and write their items at the
// range's place.  `built`: the commit is from a device-built trial's resident rows, which carry the candidates' frames.
static int commit_collect(mgpu_engine *e, Lane &ln, int n, const int *replica, const int *t, const int *m, const int *kind,
                          const double *sites, int site_stride, const int *accept, bool built, int parts, CommitPart *part_of,
                          RecipItem *items, int &n_items) {
    // one accepted candidate per replica: ln.commit_mark[replica] holds the stamp of the call that last committed there (a
    // fresh stamp per call instead of clearing n_replicas flags; exchanged atomically: the ranges below run side by side)
    if ((int)ln.commit_mark.size() != e->n_replicas) { ln.commit_mark.assign(e->n_replicas, -1); ln.commit_stamp = 0; }
    if (++ln.commit_stamp == 0x7fffffff) { std::fill(ln.commit_mark.begin(), ln.commit_mark.end(), -1); ln.commit_stamp = 1; }
    const int stamp = ln.commit_stamp;
    PartError errs[kMaxHostParts];
    n_items = 0;
    if (parts > 1) {
        for_parts(parts, [&](int q) {
            int c0, c1, k = 0;
            part_range(n, parts, q, c0, c1);
            for (int c = c0; c < c1; ++c) k += accept[c] != 0;
            part_of[q].n_acc = k;
        });
        for (int q = 0; q < parts; ++q) { part_of[q].at = n_items; n_items += part_of[q].n_acc; }
    }
    for_parts(parts, [&](int q) {
        CommitPart &P = part_of[q];
        int c0, c1, at = P.at;
        part_range(n, parts, q, c0, c1);
        for (int c = c0; c < c1; ++c) {
            if (!accept[c]) continue;
            if (kind[c] < MGPU_MOVE || kind[c] > MGPU_DELETION) { errs[q].set(c, MGPU_ERR_INVALID_ARG, "commit: unknown candidate kind"); return; }
            if (replica[c] < 0 || replica[c] >= e->n_replicas) { errs[q].set(c, MGPU_ERR_INVALID_ARG, "commit: replica out of range"); return; }
            int &mark = ln.commit_mark[replica[c]];
            int before;
            if (parts > 1) before = __atomic_exchange_n(&mark, stamp, __ATOMIC_RELAXED);     // (the exchange IS the store)
            else { before = mark; mark = stamp; }
            if (before == stamp) {
                errs[q].set(c, MGPU_ERR_INVALID_ARG, "commit: more than one accepted candidate for a replica");
                return;
            }
            if (t[c] < 0 || t[c] >= e->tp.n_res) { errs[q].set(c, MGPU_ERR_INVALID_ARG, "commit: residue type out of range"); return; }
            const int idx = replica[c] * e->tp.n_res + t[c], nm = e->h_nmol[idx];
            RecipItem it{replica[c], t[c], m[c], kind[c], -1, nm};
            if (kind[c] == MGPU_CREATION) {
                if (nm >= e->tp.cap[t[c]]) { errs[q].set(c, MGPU_ERR_CAPACITY, "commit: residue type is at mol_capacity"); return; }
                it.m = nm;  // appended at the first free slot: num_residues + 1 (monte_carlo.f90:63, create_molecule.f90:64)
                it.aux = nm + 1;
            } else {
                if (const int r = check_candidate(e, c, replica[c], t[c], m[c], true)) { errs[q].set(c, r, mgpu_last_error()); return; }
                if (kind[c] == MGPU_DELETION) it.aux = nm - 1;
            }
            if (kind[c] != MGPU_DELETION) {
                P.any_sites = true;
                it.src = c;
                it.frame = built ? ln.last_trial_frame : 0;
                // where the engine keeps molecule frames they must stay the mirror of the sites: a move / insertion given as
                // bare sites cannot update them
                if (!built && e->d_com && e->frames_ok[idx]) {
                    errs[q].set(c, MGPU_ERR_STATE, "commit: this replica holds molecule frames (mgpu_replica_set_frames): commit "
                                                   "device-built trials from the lane's resident rows, or set the molecules again");
                    return;
                }
                // the accepted sites become resident atoms: keep the replica's range flag honest
                const bool ok = sites ? sites_in_range(e, sites + (size_t)c * site_stride * 3, e->tp.n1[t[c]])
                                      : (c < (int)ln.cand_ok.size() && ln.cand_ok[c]);
                if (!ok) P.range_lost.push_back(idx);
                if (e->tp.n1[t[c]] > site_stride) { errs[q].set(c, MGPU_ERR_INVALID_ARG, "site_stride smaller than atoms_in_res"); return; }
            }
            if (kind[c] == MGPU_DELETION && built) it.frame = ln.last_trial_frame;   // (device-built: a reservoir receives the last slot)
            if (kind[c] != MGPU_MOVE) { P.new_counts.push_back(idx); P.new_counts.push_back(it.aux); }
            items[at++] = it;
        }
        if (parts == 1) n_items = at;        // (one range: counted as it went)
    });
    if (int rc = report_first(errs, parts)) return commit_refused(e, ln, n, replica, accept, errs, parts, rc);
    return MGPU_OK;
}

// Part 2a: committing the lane's last trial from its resident rows.  The trial's items are still on the device too, so the
// accept flags travel as a kernel argument and nothing is uploaded.
static int commit_from_trial(mgpu_engine *e, Lane &ln, int n, const int *replica, const int *t, const int *m, const int *kind,
                             int site_stride, const int *accept, int parts, int n_items) {
    AcceptBits bits{};
    bool same_of[kMaxHostParts];   // the caller promises the trial's candidates in the trial's order: verify
    for_parts(parts, [&](int q) {  // (the ranges end on multiples of 32 candidates: a mask word belongs to one range)
        bool same = true;
        int c0, c1;
        part_range(n, parts, q, c0, c1);
        for (int c = c0; c < c1; ++c) {
            if (!accept[c]) continue;
            const RecipItem &ti = ln.h_trial_items[c];
            same = same && ti.replica == replica[c] && ti.t == t[c] && ti.kind == kind[c] &&
                   (kind[c] == MGPU_CREATION || ti.m == m[c]);
            bits.w[c >> 5] |= 1u << (c & 31);
        }
        same_of[q] = same;
    });
    bool same = true;
    for (int q = 0; q < parts; ++q) same = same && same_of[q];
    if (!same) return set_error(MGPU_ERR_INVALID_ARG, "commit_submit: candidates differ from the lane's last trial");
    // The trial stored the A + delta of its candidates into their replicas' other buffers, and nothing has touched those
    // since (alt_owner still holds the trial's stamp for every accepted one): switch buffers.  Otherwise A + delta again.
    bool switch_ok = ln.trial_alt && !e->commit_pass;
    for (int c = 0; c < n && switch_ok; ++c)
        switch_ok = !accept[c] || __atomic_load_n(&e->alt_owner[replica[c]], __ATOMIC_RELAXED) == ln.trial_stamp;
    ln.accept_share = (double)n_items / n;
    int rc;
    if (switch_ok) {
        if ((rc = launch_commit_switch(e, ln, ln.d_trial_items, n, site_stride, bits))) return rc;
        e->a_switched = true;
    } else if ((rc = launch_recip(e, ln, ln.d_trial_items, n, ln.trial_n1_max, site_stride, true, e->d_A, nullptr, nullptr, &bits)))
        return rc;
    // applied once: a second commit_submit(sites = NULL) must not find these rows "resident" again
    ln.forget_trial();
    return MGPU_OK;
}

// Part 2b: committing uploaded items (and, where the caller gave sites, uploaded rows).
static int commit_from_items(mgpu_engine *e, Lane &ln, int n, const int *t, const double *sites, int site_stride, RecipItem *items,
                             int n_items, bool any_sites) {
    int rc;
    recip_groups(e, items, n_items, ln.recip_groups, ln.recip_order);
    if (!ln.recip_order.empty()) {
        const std::vector<RecipItem> as_accepted(items, items + n_items);
        for (int s = 0; s < n_items; ++s) items[s] = as_accepted[ln.recip_order[s]];
    }
    if ((rc = ln.d_items2.reserve((size_t)n_items * sizeof(RecipItem)))) return rc;
    HIP_TRY(hipMemcpyAsync(ln.d_items2.p, items, (size_t)n_items * sizeof(RecipItem), hipMemcpyHostToDevice, ln.stream));
    if (any_sites && sites) {
        const size_t site_bytes = (size_t)n * site_stride * 3 * sizeof(double);
        ln.forget_trial();      // (their rows are about to be overwritten)
        std::memcpy(ln.h_commit.p, sites, site_bytes);
        if (any_frozen(e, n, t)) permute_frozen_rows(e, (double *)ln.h_commit.p, n, site_stride, t);
        if ((rc = ln.d_sites.reserve(site_bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(ln.d_sites.p, ln.h_commit.p, site_bytes, hipMemcpyHostToDevice, ln.stream));
    }
    if (!ln.commit_staged_ev) HIP_TRY(hipEventCreateWithFlags(&ln.commit_staged_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ln.commit_staged_ev, ln.stream));
    ln.commit_staged = true;
    // each accepted candidate in the form of its own type, as in its trial (the items touch one replica each: any order)
    for (const RecipGroup &g : ln.recip_groups)
        if ((rc = launch_recip(e, ln, (const RecipItem *)ln.d_items2.p + g.first, g.n, g.n1_max, site_stride, true, e->d_A, nullptr)))
            return rc;
    return MGPU_OK;
}

// Queue the commit of the accepted candidates on a lane (no synchronisation).  The host-side
// molecule counts are updated immediately; the device applies them in stream order.
// reuse_sites: `sites` may be NULL, meaning "the rows the lane's last trial_submit uploaded" (same
// candidates, same order), which are still resident in the lane's device scratch.
static int commit_submit_impl(mgpu_engine *e, Lane &ln, int n, const int *replica, const int *t, const int *m,
                              const int *kind, const double *sites, int site_stride, const int *accept,
                              bool reuse_sites = false) {
    int rc;
    const size_t site_bytes = sites ? (size_t)n * site_stride * 3 * sizeof(double) : 0;
    if (ln.n_submitted != 0) return set_error(MGPU_ERR_STATE, "commit_submit: wait for the lane's trial first");
    ln.dirty = true;
    const bool built = !sites && reuse_sites && ln.last_trial_built && n == ln.last_trial_n;
    if (built) site_stride = ln.last_trial_stride;
    // the pinned staging block may still feed the H2D copy of the lane's previous commit
    if (ln.commit_staged) {
        HIP_TRY(hipEventSynchronize(ln.commit_staged_ev));
        ln.commit_staged = false;
    }
    if ((rc = ln.h_commit.reserve(site_bytes + (size_t)n * sizeof(RecipItem)))) return rc;
    RecipItem *items = (RecipItem *)((char *)ln.h_commit.p + site_bytes);
    const int parts = host_parts(e, n);
    CommitPart part_of[kMaxHostParts];
    int n_items;
    if ((rc = commit_collect(e, ln, n, replica, t, m, kind, sites, site_stride, accept, built, parts, part_of, items, n_items))) return rc;
    bool any_sites = false;
    for (int q = 0; q < parts; ++q) any_sites = any_sites || part_of[q].any_sites;
    if (n_items == 0) {
        if (!sites && reuse_sites) ln.accept_share = 0.0;
        return MGPU_OK;
    }
    if (any_sites && !sites && !reuse_sites) return set_error(MGPU_ERR_INVALID_ARG, "commit_candidates: sites is null");
    const bool from_trial = !sites && reuse_sites && n == ln.last_trial_n && ln.d_trial_items && n <= 32 * kAcceptWords &&
                            recip_by_rows(e, ln.trial_n1_max);
    if ((rc = from_trial ? commit_from_trial(e, ln, n, replica, t, m, kind, site_stride, accept, parts, n_items)
                         : commit_from_items(e, ln, n, t, sites, site_stride, items, n_items, any_sites)))
        return rc;
    // the committed replicas' other buffers hold no trial's A + delta for their new state
    for (int c = 0; c < n; ++c)
        if (accept[c]) alt_forget(e, replica[c]);
    ln.trial_alt = false;
    for (int q = 0; q < parts; ++q) {
        const std::vector<int> &new_counts = part_of[q].new_counts;
        for (size_t i = 0; i < new_counts.size(); i += 2) e->h_nmol[new_counts[i]] = new_counts[i + 1];
        for (int idx : part_of[q].range_lost) e->in_range[idx] = 0;
    }
    if (e->any_frozen)
        for (int c = 0; c < n; ++c)
            if (accept[c]) frozen_changed(e, replica[c], t[c]);
    return MGPU_OK;
}

static int check_lane(const mgpu_engine *e, int lane) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (lane < 0 || lane >= kLanes) return set_error(MGPU_ERR_INVALID_ARG, "lane out of range");
    return MGPU_OK;
}

int mgpu_lane_site_buffer(mgpu_engine *e, int lane, int n_max, int site_stride, double **sites) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n_max < 1 || site_stride < 1 || !sites) return set_error(MGPU_ERR_INVALID_ARG, "lane_site_buffer: bad argument");
    if ((rc = use_device(e))) return rc;
    Lane &ln = e->lanes[lane];
    if (ln.n_submitted != 0) return set_error(MGPU_ERR_STATE, "lane_site_buffer: the lane holds an un-waited trial");
    // a regrown block would leave the previous trial's item image dangling
    ln.forget_trial();
    // sized for the largest trial shape the lane accepts for n_max candidates (lane_site_buffer_bytes, mgpu_internal.h)
    if ((rc = ln.h_in.reserve(lane_site_buffer_bytes(n_max, site_stride)))) return rc;
    ln.h_in_lent = true;
    *sites = (double *)ln.h_in.p;
    return MGPU_OK;
}

int mgpu_trial_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m,
                      const double *sites, int site_stride) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n <= 0 || !replica || !t || !m || !sites) return set_error(MGPU_ERR_INVALID_ARG, "trial_submit: bad argument");
    if ((rc = use_device(e))) return rc;
    return trial_submit_impl(e, e->lanes[lane], n, replica, t, m, nullptr, sites, site_stride);
}

int mgpu_gcmc_trial_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m,
                           const int *kind, const double *sites, int site_stride) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n <= 0 || !replica || !t || !m || !kind || !sites) return set_error(MGPU_ERR_INVALID_ARG, "gcmc_trial_submit: bad argument");
    if ((rc = use_device(e))) return rc;
    return trial_submit_impl(e, e->lanes[lane], n, replica, t, m, kind, sites, site_stride);
}

// the candidate kinds of a device-built trial from its move codes, into ln.build_kind; `who` heads the error
static int build_kinds(Lane &ln, int n, const int *move, const char *who) {
    ln.build_kind.resize(n);
    for (int c = 0; c < n; ++c) {
        if (move[c] < 1 || move[c] > 4) return set_error(MGPU_ERR_INVALID_ARG, std::string(who) + ": unknown move code");
        ln.build_kind[c] = move[c] <= 2 ? MGPU_MOVE : (move[c] == 3 ? MGPU_CREATION : MGPU_DELETION);
    }
    return MGPU_OK;
}

int mgpu_move_trial_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m, const int *move,
                           const double *u, double translation_step, double rotation_step) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n <= 0 || !replica || !t || !m || !move || !u) return set_error(MGPU_ERR_INVALID_ARG, "move_trial_submit: bad argument");
    if (e->bx.triclinic && !e->tri_moves) return set_error(MGPU_ERR_STATE, "move_trial_submit: orthorhombic boxes only");
    if ((rc = use_device(e))) return rc;
    Lane &ln = e->lanes[lane];
    if ((rc = build_kinds(ln, n, move, "move_trial_submit"))) return rc;
    const TrialBuild build{move, u, translation_step, rotation_step};
    return trial_submit_impl(e, ln, n, replica, t, m, ln.build_kind.data(), nullptr, 0, &build);
}

int mgpu_move_trial_decide_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m, const int *move,
                                  const double *u, double translation_step, double rotation_step, const double *accept_u,
                                  const double *accept_pref, double temperature) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n <= 0 || !replica || !t || !m || !move || !u || !accept_u || !accept_pref)
        return set_error(MGPU_ERR_INVALID_ARG, "move_trial_decide_submit: bad argument");
    if (e->bx.triclinic && !e->tri_moves) return set_error(MGPU_ERR_STATE, "move_trial_decide_submit: orthorhombic boxes only");
    if ((rc = use_device(e))) return rc;
    Lane &ln = e->lanes[lane];
    if ((rc = build_kinds(ln, n, move, "move_trial_decide_submit"))) return rc;
    const TrialBuild build{move, u, translation_step, rotation_step};
    const TrialDecide dec{accept_u, accept_pref, temperature};
    return trial_submit_impl(e, ln, n, replica, t, m, ln.build_kind.data(), nullptr, 0, &build, &dec);
}

int mgpu_gcmc_trial_decide_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m,
                                  const int *kind, const double *sites, int site_stride, const double *accept_u,
                                  const double *accept_pref, double temperature) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n <= 0 || !replica || !t || !m || !kind || !sites || !accept_u || !accept_pref)
        return set_error(MGPU_ERR_INVALID_ARG, "gcmc_trial_decide_submit: bad argument");
    if ((rc = use_device(e))) return rc;
    const TrialDecide dec{accept_u, accept_pref, temperature};
    return trial_submit_impl(e, e->lanes[lane], n, replica, t, m, kind, sites, site_stride, nullptr, &dec);
}

int mgpu_trial_decide_wait(mgpu_engine *e, int lane, double *old_energy, double *new_energy, int *accepted) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (!old_energy || !new_energy || !accepted) return set_error(MGPU_ERR_INVALID_ARG, "trial_decide_wait: null output");
    if ((rc = use_device(e))) return rc;
    return trial_wait_impl(e, e->lanes[lane], old_energy, new_energy, 5, accepted);
}

int mgpu_gcmc_trial_wait(mgpu_engine *e, int lane, double *old_energy, double *new_energy) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (!old_energy || !new_energy) return set_error(MGPU_ERR_INVALID_ARG, "gcmc_trial_wait: null output");
    if ((rc = use_device(e))) return rc;
    return trial_wait_impl(e, e->lanes[lane], old_energy, new_energy, 5);
}

int mgpu_trial_wait(mgpu_engine *e, int lane, double *old_energy, double *new_energy) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (!old_energy || !new_energy) return set_error(MGPU_ERR_INVALID_ARG, "trial_wait: null output");
    if ((rc = use_device(e))) return rc;
    return trial_wait_impl(e, e->lanes[lane], old_energy, new_energy, 3);
}

int mgpu_commit_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m, const int *kind,
                       const double *sites, int site_stride, const int *accept) {
    int rc = check_lane(e, lane);
    if (rc) return rc;
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !kind || !accept) return set_error(MGPU_ERR_INVALID_ARG, "commit_submit: bad argument");
    if ((rc = use_device(e))) return rc;
    Lane &ln = e->lanes[lane];
    const bool reuse = (sites == nullptr) && ln.last_trial_n == n && (ln.last_trial_stride == site_stride || ln.last_trial_built);
    return commit_submit_impl(e, ln, n, replica, t, m, kind, sites, site_stride, accept, reuse);
}

int mgpu_trial_energy_candidates(mgpu_engine *e, int n, const int *replica, const int *t, const int *m,
                                 const double *sites, int site_stride, double *old_energy, double *new_energy) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !sites || !old_energy || !new_energy)
        return set_error(MGPU_ERR_INVALID_ARG, "trial_energy_candidates: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    if ((rc = trial_submit_impl(e, e->lanes[0], n, replica, t, m, nullptr, sites, site_stride))) return rc;
    return trial_wait_impl(e, e->lanes[0], old_energy, new_energy, 3);
}

int mgpu_commit_candidates(mgpu_engine *e, int n, const int *replica, const int *t, const int *m, const int *kind,
                           const double *sites, int site_stride, const int *accept) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (n == 0) return MGPU_OK;
    if (n < 0 || !replica || !t || !m || !kind || !accept) return set_error(MGPU_ERR_INVALID_ARG, "commit_candidates: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;
    if ((rc = commit_submit_impl(e, e->lanes[0], n, replica, t, m, kind, sites, site_stride, accept))) return rc;
    return sync_stream(e);
}


int mgpu_set_triclinic_moves(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;      // (no trial or window in flight sees the switch move)
    e->tri_moves = on != 0;
    return MGPU_OK;
}

int mgpu_set_host_team(mgpu_engine *e, int n_threads) {
    if (!e || n_threads < 1) return set_error(MGPU_ERR_INVALID_ARG, "set_host_team: bad argument");
    e->host_team = std::min(n_threads, kMaxHostParts);
    return MGPU_OK;
}


}  // extern "C"
