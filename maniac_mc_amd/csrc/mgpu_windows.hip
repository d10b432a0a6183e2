// One-launch windows (include/maniac_gpu.h): a window of speculative steps of ONE chain (mgpu_chain_window) and one step of a
// FARM of chains (mgpu_farm_window_*): evaluation, acceptance and commit in a single kernel, results through pinned host
// memory the host polls.
#include "mgpu_engine.h"

#include <map>

namespace mgpu {

// The engine's Topo in device memory (the window kernels index it by residue types they LOAD: as a by-value kernel argument
// the compiler would copy all of it into every lane's scratch); refreshed when the frames' buffers appear.
int chain_topo(mgpu_engine *e, const Topo **d_topo) {
    mgpu_engine::Chain &ch = e->chain;
    if (!ch.d_topo) {
        HIP_TRY(hipMalloc((void **)&ch.d_topo, sizeof(Topo)));
        ch.topo_stale = true;
    }
    if (ch.topo_stale) {
        for (auto &ln : e->lanes) HIP_TRY(hipStreamSynchronize(ln.stream));
        HIP_TRY(hipMemcpy(ch.d_topo, &e->tp, sizeof(Topo), hipMemcpyHostToDevice));
        ch.topo_stale = false;
    }
    *d_topo = ch.d_topo;
    return MGPU_OK;
}

// Every replica's current A(k) back into the primary buffer d_A (farm windows and commits by switching move a replica between
// d_A and d_A_alt): drains the lanes, one small launch, a synchronise.  Windows still un-waited keep their results in host memory.
// Afterwards no replica's other buffer holds anything a commit may switch to.
int normalize_A(mgpu_engine *e) {
    e->a_switched = false;
    if (!e->d_A_alt) return MGPU_OK;
    for (auto &ln : e->lanes) HIP_TRY(hipStreamSynchronize(ln.stream));
    hipLaunchKernelGGL(farm_normalize_kernel, dim3(e->n_replicas), dim3(kBlock), 0, e->lanes[0].stream, e->d_acur, e->d_A,
                       (const double2 *)e->d_A_alt, e->n_slots);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->lanes[0].stream));
    alt_forget(e, -1);
    return MGPU_OK;
}

// The A(k) double buffer, on first use: R x n_slots complex entries more, every replica current in d_A
int alt_reserve(mgpu_engine *e) {
    std::lock_guard<std::mutex> lock(e->alt_mu);
    if (e->d_A_alt) return MGPU_OK;
    double2 *alt = nullptr;
    int *cur = nullptr;
    HIP_TRY(hipMalloc((void **)&alt, (size_t)e->n_replicas * e->n_slots * sizeof(double2)));
    HIP_TRY(hipMalloc((void **)&cur, (size_t)e->n_replicas * sizeof(int)));
    HIP_TRY(hipMemset(cur, 0, (size_t)e->n_replicas * sizeof(int)));
    HIP_TRY(hipDeviceSynchronize());
    e->d_acur = cur;
    e->d_A_alt = alt;
    return MGPU_OK;
}

void alt_forget(mgpu_engine *e, int replica) {
    if (e->alt_owner.empty()) return;
    if (replica >= 0) { __atomic_store_n(&e->alt_owner[replica], 0ull, __ATOMIC_RELAXED); return; }
    for (auto &o : e->alt_owner) __atomic_store_n(&o, 0ull, __ATOMIC_RELAXED);
}

// A replica whose state is rewritten (set_molecules / set_frames / set_num_molecules, the destination of replica_copy)
// waits for no decision of an earlier step: its stall flag goes.  The callers have drained every lane.
int farm_clear_stall(mgpu_engine *e, int replica) {
    if (e->farm.d_stalled) HIP_TRY(hipMemset(e->farm.d_stalled + replica, 0, sizeof(int)));
    mgpu_engine::Run &rn = e->run;
    if (rn.open && rn.replica == replica) {                   // an open chain run of the replica: the same
        HIP_TRY(hipMemset(&rn.d_state->stalled, 0, sizeof(int)));
        rn.stalled_at = -1;
        rn.dev_stalled = false;
    }
    return MGPU_OK;
}

void chain_run_release(mgpu_engine *e) {
    mgpu_engine::Run &rn = e->run;
    for (void *p : {(void *)rn.h_ring, (void *)rn.h_gc, (void *)rn.h_pushed, (void *)rn.h_out, (void *)rn.h_step_tag, (void *)rn.h_launch})
        if (p) (void)hipHostFree(p);
    for (void *p : {(void *)rn.d_state, (void *)rn.d_ring, (void *)rn.d_gc, (void *)rn.d_part, (void *)rn.d_alt, (void *)rn.d_res, (void *)rn.d_ticket})
        if (p) (void)hipFree(p);
    rn = mgpu_engine::Run{};
}

int wait_for_tag(hipStream_t stream, const volatile unsigned long long *tag, int n, unsigned long long seq, long long first_check,
                 long long check_every, const char *what) {
    long long spins = 0;
    for (int c = 0; c < n; ++c) {
        while (tag[c] != seq) {
            __builtin_ia32_pause();
            if (++spins >= first_check && (spins % check_every) == 0) {
                // long past any window's run time: make sure the stream is still alive
                const hipError_t q = hipStreamQuery(stream);
                if (q == hipSuccess && tag[c] != seq) return set_error(MGPU_ERR_HIP, std::string(what) + ": the kernel finished without publishing its results");
                if (q != hipSuccess && q != hipErrorNotReady) return set_error(MGPU_ERR_HIP, std::string(what) + ": " + hipGetErrorString(q));
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return MGPU_OK;
}

// ---- what the three one-launch paths take, and the launch they share --------------------------

// e->win: the k role a window (farm or, for a type of more than kMaxFusedSitesWide sites, single-chain) gives a row of residue
// type t -- the form recip_plan picks for the type alone, as the batched path's per-type launches do (recip_groups) -- and the
// dynamic LDS that role needs.  kWindowNone: windows do not take the type (site-major types, i.e. molecules of kFarmWideSites
// sites or more, frozen ones among them; a molecule of <= kMaxFusedSitesWide sites whose type does not take the row form; a larger
// one in a triclinic box -- what the image-search WIDE instances would take of such a type goes to take_tri, read by the
// single-chain paths under mgpu_chain_set_wide_triclinic and by farm windows under mgpu_farm_set_wide_triclinic -- or whose type
// takes the per-k or the tiled matrix-unit form).  Everything read here is fixed when the engine is created.
void window_types_build(mgpu_engine *e) {
    mgpu_engine::WindowTypes &w = e->win;
    w = mgpu_engine::WindowTypes{};
    w.k_lds_one = recip_rows_lds_bytes(e, 1);
    w.rows_one = recip_by_rows(e, 1);
    for (int t = 0; t < e->tp.n_res; ++t) {
        const int n1 = e->tp.n1[t];
        const bool wide = n1 > kMaxFusedSitesWide;
        if (!wide) w.k_lds[t] = window_k_lds_bytes(false, recip_rows_lds_bytes(e, n1));   // (a narrow row's k role is the row form's)
        if (e->tp.site_major[t] || n1 >= kFarmWideSites) continue;
        const bool tri_wide = wide && e->bx.triclinic;
        const RecipPlan p = recip_plan(e, n1, true);
        if (p.form == MGPU_RECIP_FORM_ROWS) {
            w.k_lds[t] = window_k_lds_bytes(wide, recip_rows_lds_bytes(e, n1));
        } else if (wide && (p.form == MGPU_RECIP_FORM_WIDE_VECTOR || p.form == MGPU_RECIP_FORM_WIDE_MFMA)) {
            // launch_recip's tables (2 n1 site-states), or one tile of site-states
            w.kform[t] = (signed char)(p.mfma_tile ? kFarmFormWideMfma : kFarmFormWideVector);
            w.wide_rpt[t] = p.wide_rpt; w.wide_nss[t] = p.wide_nss;
            w.k_lds[t] = window_k_lds_bytes(true, p.wide_lds);
        } else {
            continue;
        }
        w.k_lds_max_tri = std::max(w.k_lds_max_tri, w.k_lds[t]);
        if (tri_wide) { w.take_tri[t] = kWindowWide; continue; }
        w.take[t] = wide ? kWindowWide : kWindowNarrow;
        w.k_lds_max = std::max(w.k_lds_max, w.k_lds[t]);         // (every type a row may carry)
    }
}

// What a path admits, from e->win and the switches laid over it (mgpu_chain_set_wide, mgpu_set_triclinic_moves,
// mgpu_chain_run_set_triclinic, reservoirs).  capacity: candidates of a single-chain window, chains of a farm window, steps of a
// chain-run launch; 0 where the path does not apply --
//   every path: an active type it does not take (a narrow type off the row form, a site-major one, one of more than
//     kMaxFusedSitesWide sites unless the path has WIDE instances, they are on and windows take the type), a Coulomb table or a
//     resolver beyond 64 KiB, WIDE LDS beyond its budget;
//   farm windows and chain runs: a triclinic box whose engine has not switched device-built moves on;
//   chain runs (no such instance of chain_run_kernel exists): reservoirs, and a triclinic box unless triclinic runs are on; a type
//     of more than kMaxFusedSitesWide sites unless WIDE runs are on (mgpu_chain_run_set_wide: refused for an engine with a
//     reservoir, and for a triclinic box unless mgpu_chain_set_wide_triclinic is on);
//   single-chain windows and chain runs under mgpu_chain_set_wide_triclinic: a type of 6..63 sites of a triclinic box is taken as
//     take_tri says (the TRI x WIDE instances); farm windows read it under a switch of their own, mgpu_farm_set_wide_triclinic,
//     and neither switch gives the other's paths anything.
//     (Grand-canonical runs, mgpu_chain_run_set_gc, are admitted exactly where runs are: the switch is refused for a triclinic box
//     whose triclinic runs are off and for an engine with a reservoir, and the GC instances' dynamic LDS is window_lds_bytes(kPathRun, ...) -- their k role, pair
//     role and resolver stage what the NVT instances stage; what they add is 16 double2 of static LDS.)
// rides[t]: a record of type t may travel (a single-chain window takes any row of <= kMaxFusedSitesWide sites; a run any active type).
struct WindowAdmission {
    int capacity = 0;
    bool rides[kMaxRes] = {};
};
// the image-search WIDE instances serve this path of this engine (farm windows: mgpu_farm_set_wide_triclinic; the single-chain
// paths: mgpu_chain_set_wide_triclinic), and whether the path's WIDE instances, once on, take type t
static bool window_tri_wide(const mgpu_engine *e, WindowPath path) {
    return e->bx.triclinic && (path != kPathFarm ? e->wide_tri : e->farm_wide_tri);
}
static bool window_takes_wide(const mgpu_engine *e, WindowPath path, int t) {
    return e->win.take[t] == kWindowWide || (window_tri_wide(e, path) && e->win.take_tri[t] == kWindowWide);
}
static WindowAdmission window_admission(const mgpu_engine *e, WindowPath path) {
    const mgpu_engine::WindowTypes &w = e->win;
    const bool wide_on = path == kPathFarm || (path == kPathChain && e->chain.wide) || (path == kPathRun && e->run.wide);
    const bool tri_wide_on = window_tri_wide(e, path);
    WindowAdmission a;
    bool ok = true, wide = false;
    for (int t = 0; t < e->tp.n_res; ++t) {
        const bool takes = w.take[t] == kWindowNarrow || (window_takes_wide(e, path, t) && wide_on);
        a.rides[t] = path == kPathRun ? e->is_active[t] != 0 : (takes || (path == kPathChain && e->tp.n1[t] <= kMaxFusedSitesWide));
        if (!e->is_active[t]) continue;
        ok = ok && takes;
        wide = wide || window_takes_wide(e, path, t);
    }
    if (path != kPathChain && e->bx.triclinic && !e->tri_moves) ok = false;
    if (path == kPathRun && (e->rsv_any || (e->bx.triclinic && !e->run.triclinic))) ok = false;
    if (path == kPathChain && !w.rows_one) ok = false;
    const int nsplit = e->pair_nsplit;
    if (!window_lds_fits(false, window_lds_bytes(path, false, e->coul_bytes, 0, 0, nsplit))) ok = false;
    if (wide && !window_lds_fits(true, window_lds_bytes(path, true, e->coul_bytes, tri_wide_on ? w.k_lds_max_tri : w.k_lds_max, 0, nsplit))) ok = false;
    if (!ok) return a;
    // (single-chain windows, runs: the resolving workgroup stages every split partial in LDS, 2 entries per step at most)
    a.capacity = path == kPathFarm ? std::min(kFarmMaxChains, e->n_replicas)
                                   : std::max(0, std::min(path == kPathChain ? kChainMaxCand : kRunMaxK, chain_window_steps_by_lds(nsplit)));
    return a;
}

// a launch's dynamic LDS (mgpu_internal.h): `k_rows` = the largest k role among the narrow rows it carries; a WIDE launch takes
// the largest over every type a row may carry
static size_t window_lds(const mgpu_engine *e, WindowPath path, bool wide, size_t k_rows, int count) {
    const size_t k_bytes = wide ? (window_tri_wide(e, path) ? e->win.k_lds_max_tri : e->win.k_lds_max) : std::max(e->win.k_lds_one, k_rows);
    return window_lds_bytes(path, wide, e->coul_bytes, k_bytes, count, e->pair_nsplit);
}

// what the WIDE instances read besides: the k role's form per residue type and its tile, the rows' first tasks, where the pair
// role's slabs start in dynamic LDS
static void wide_args(const mgpu_engine *e, const int **row_first, int *wide_at, signed char *kform, int *wide_rpt, int *wide_nss) {
    *row_first = e->d_row_first;
    *wide_at = (int)chain_wide_pair_at(e->coul_bytes);
    std::memcpy(kform, e->win.kform, sizeof(e->win.kform));
    std::memcpy(wide_rpt, e->win.wide_rpt, sizeof(e->win.wide_rpt));
    std::memcpy(wide_nss, e->win.wide_nss, sizeof(e->win.wide_nss));
}

// Beyond 64 KiB of dynamic LDS a kernel opts in (gfx950: up to 160 KiB per workgroup); only the WIDE instances get here.  The
// limit belongs to the kernel function, not to an engine: the most each family has asked for on each device is kept for the
// whole process, and only a larger size sets the attribute again.  each(f) calls f(kernel) for every instance of the family.
enum LdsFamily { kLdsChainWide, kLdsFarmWide, kLdsRunWide, kLdsFamilies };
static std::mutex g_lds_opt_mu;
static std::map<int, size_t> g_lds_opted[kLdsFamilies];       // [family][device]
template <class Each>
static int lds_opt_in(int device, LdsFamily family, size_t lds, Each &&each) {
    if (lds <= kLdsDefaultMax) return MGPU_OK;
    std::lock_guard<std::mutex> lock(g_lds_opt_mu);
    size_t &opted = g_lds_opted[family][device];
    if (lds <= opted) return MGPU_OK;
    hipError_t err = hipSuccess;
    each([&](auto kernel) {
        if (err == hipSuccess) err = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    if (err != hipSuccess)
        return set_error(MGPU_ERR_HIP, std::string("hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds): ") + hipGetErrorString(err));
    opted = lds;
    return MGPU_OK;
}

// the launch of any instance of the three kernels: the engine's arguments, then the path's own
template <class Kernel, class Args>
static void window_launch(Kernel kernel, const mgpu_engine *e, const Topo *d_topo, int grid, size_t lds, hipStream_t stream, const Args &g) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kChainBlock), lds, stream, d_topo, e->bx, e->d_pos, e->d_nmol, e->d_res_q, e->d_res_atype,
                       e->d_pair_tab, e->d_coul_tab, e->d_trj, e->d_tw, e->n_rtasks, e->d_rrows, e->n_rrows, e->d_A, g);
}

// a result row "five old | five new" (non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb) into the caller's row c
static void copy_energy_rows(double *old_energy, double *new_energy, size_t c, const double *row) {
    std::memcpy(old_energy + 5 * c, row, 5 * sizeof(double));
    std::memcpy(new_energy + 5 * c, row + 5, 5 * sizeof(double));
}

// the device has committed (or is committing, behind the tag) a step of `kind` on (replica, t): the host mirrors follow.
// in_range_ok = false: the new sites may lie outside the fast fold's range (an as-written deletion moves resident atoms only:
// the range flag stands)
static void mirror_accepted(mgpu_engine *e, int replica, int t, int kind, bool in_range_ok) {
    const size_t idx = (size_t)replica * e->tp.n_res + t;
    if (kind == MGPU_CREATION) e->h_nmol[idx] += 1;
    if (kind == MGPU_DELETION) e->h_nmol[idx] -= 1;
    if (kind != MGPU_DELETION && !in_range_ok) e->in_range[idx] = 0;
    frozen_changed(e, replica, t);
}

}  // namespace mgpu

extern "C" {

// ---- single-chain windows --------------------------------------------------------------------

int mgpu_chain_set_wide(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    e->chain.wide = on != 0;
    return MGPU_OK;
}

int mgpu_chain_set_wide_triclinic(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    // every refusal leaves the switch as it was
    if (!e->bx.triclinic) return set_error(MGPU_ERR_STATE, "chain_set_wide_triclinic: the box is orthorhombic");
    if (e->run.open) return set_error(MGPU_ERR_STATE, "chain_set_wide_triclinic: a run is open");
    // (WIDE runs of a triclinic box stand on this switch: mgpu_chain_run_set_wide)
    if (!on && e->run.wide) return set_error(MGPU_ERR_STATE, "chain_set_wide_triclinic: WIDE runs are on (mgpu_chain_run_set_wide)");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;      // (no trial or window in flight sees the switch move)
    e->wide_tri = on != 0;
    return MGPU_OK;
}

int mgpu_chain_window_capacity(const mgpu_engine *e, int *max_candidates) {
    if (!e || !max_candidates) return set_error(MGPU_ERR_INVALID_ARG, "chain_window_capacity: null argument");
    *max_candidates = window_admission(e, kPathChain).capacity;
    return MGPU_OK;
}

int mgpu_chain_set_margin(mgpu_engine *e, double relative_margin) {
    if (!e || !(relative_margin >= 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "chain_set_margin: bad argument");
    e->chain.margin = relative_margin;
    return MGPU_OK;
}

int mgpu_chain_set_timing(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    e->chain.timing = on != 0;
    return MGPU_OK;
}

// Stage times of the LAST window in microseconds since its first workgroup started (100 MHz wall clock of the device):
//   us[0..3]   k role of candidate 0: start, phase tables built, k sweep summed, at the ticket
//   us[4..7]   first pair workgroup:  start, Coulomb table staged, its work units swept, at the ticket
//   us[8..14]  resolving workgroup:   last ticket drawn, acquire fence, partials reduced, decided, tag published,
//                                     commit tables built, commit done (the last two 0 when nothing was accepted)
int mgpu_chain_get_timing(mgpu_engine *e, double us[15]) {
    if (!e || !us) return set_error(MGPU_ERR_INVALID_ARG, "chain_get_timing: null argument");
    if (!e->chain.h_out) return set_error(MGPU_ERR_STATE, "chain_get_timing: no window has run");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->lanes[0].stream));      // the commit's stamps are written behind the tag
    const long long *ts = (const long long *)(e->chain.h_out + 10 * kChainMaxCand + 2);
    const long long t0 = std::min(ts[0], ts[kChainStamps]);
    const int first = ((const int *)(e->chain.h_out + 10 * (size_t)kChainMaxCand))[0];
    int k = 0;
    for (int i = 0; i < 4; ++i) us[k++] = (double)(ts[i] - t0) * 0.01;
    for (int i = 0; i < 4; ++i) us[k++] = (double)(ts[kChainStamps + i] - t0) * 0.01;
    for (int i = 0; i < 7; ++i) us[k++] = (i >= 5 && first < 0) ? 0.0 : (double)(ts[2 * kChainStamps + i] - t0) * 0.01;
    return MGPU_OK;
}

int mgpu_chain_get_stats(const mgpu_engine *e, long long *windows, long long *undecided) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (windows) *windows = e->chain.windows;
    if (undecided) *undecided = e->chain.undecided;
    return MGPU_OK;
}

int mgpu_chain_window(mgpu_engine *e, int replica, int n, const int *t, const int *m, const int *kind, const int *link,
                      const double *sites, int site_stride, const double *accept_u, const double *accept_pref,
                      double temperature, double recip_energy, double *old_energy, double *new_energy, int *first_accepted,
                      int *undecided) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (!t || !m || !kind || !link || !sites || !accept_u || !accept_pref || !old_energy || !new_energy || !first_accepted || !undecided)
        return set_error(MGPU_ERR_INVALID_ARG, "chain_window: null argument");
    const WindowAdmission adm = window_admission(e, kPathChain);
    const int n_max = adm.capacity;
    if (n_max == 0) return set_error(MGPU_ERR_STATE, "chain_window: not available for this engine (mgpu_chain_window_capacity)");
    if (n < 1 || n > n_max) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: window size out of range");
    if (replica < 0 || replica >= e->n_replicas) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: replica out of range");
    if (!(temperature > 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: temperature must be positive");
    int rc = use_device(e);
    if (rc) return rc;
    Lane &ln = e->lanes[0];
    if (ln.n_submitted != 0) return set_error(MGPU_ERR_STATE, "chain_window: lane 0 still holds an un-waited trial");
    mgpu_engine::Chain &ch = e->chain;
    if (!ch.h_tag) {
        HIP_TRY(hipHostMalloc((void **)&ch.h_out, sizeof(double) * (10 * kChainMaxCand + 2 + 3 * kChainStamps), hipHostMallocCoherent));
        std::memset(ch.h_out, 0, sizeof(double) * (10 * kChainMaxCand + 2 + 3 * kChainStamps));
        HIP_TRY(hipHostMalloc((void **)&ch.h_tag, 64, hipHostMallocCoherent));
        *ch.h_tag = 0;
        HIP_TRY(hipMalloc((void **)&ch.d_res, sizeof(ChainResult) * kChainMaxCand));
        HIP_TRY(hipMalloc((void **)&ch.d_part, sizeof(double2) * 2 * kChainMaxCand * (size_t)e->pair_nsplit));
        HIP_TRY(hipMalloc((void **)&ch.d_alt, sizeof(double2) * kChainMaxCand * (size_t)e->n_slots));
        HIP_TRY(hipMalloc((void **)&ch.d_ticket, sizeof(int)));
        HIP_TRY(hipMemset(ch.d_ticket, 0, sizeof(int)));
        HIP_TRY(hipDeviceSynchronize());
    }
    if (ch.wide && !ch.h_rows) {
        // the rows of wide windows: two blocks, taken in turn -- the kernel of the window before may still read its accepted
        // row for the commit (behind the tag) while the next window's rows are written; the launches of a stream run in order
        HIP_TRY(hipHostMalloc((void **)&ch.h_rows, 2 * kChainWideRowsBytes, hipHostMallocCoherent));
    }
    const Topo *d_topo = nullptr;
    if ((rc = chain_topo(e, &d_topo))) return rc;
    if (e->a_switched && (rc = normalize_A(e))) return rc;      // (the window reads and writes d_A)
    alt_forget(e, replica);
    // ---- the window travels in the kernel arguments
    ChainArgs g{};
    bool fast = replica_in_range(e, replica);
    char cand_ok[kChainMaxCand];
    int n_ent = 0;
    size_t k_rows = 0;
    bool wide = false;
    double *wide_rows = ch.h_rows ? ch.h_rows + ((ch.seq + 1) & 1) * (kChainWideRowsBytes / sizeof(double)) : nullptr;
    for (int c = 0; c < n; ++c) {
        const int k = kind[c];
        if (k < MGPU_MOVE || k > MGPU_DELETION) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: unknown candidate kind");
        if (t[c] < 0 || t[c] >= e->tp.n_res) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: residue type out of range");
        const int n1 = e->tp.n1[t[c]];
        const bool wide_row = n1 > kMaxFusedSitesWide;
        if (n1 > site_stride || !adm.rides[t[c]])
            return set_error(MGPU_ERR_INVALID_ARG, "chain_window: molecule too large for the one-launch path");
        wide = wide || wide_row;
        const size_t idx = (size_t)replica * e->tp.n_res + t[c];
        if (e->d_com && e->frames_ok[idx])
            return set_error(MGPU_ERR_STATE, "chain_window: this replica holds molecule frames (mgpu_replica_set_frames)");
        const int lk = link[c];
        if (lk < -2 || lk >= n) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: bad link");
        if (lk >= 0 && (k != MGPU_DELETION || link[lk] != -2 || kind[lk] != MGPU_CREATION || t[lk] != t[c]))
            return set_error(MGPU_ERR_INVALID_ARG, "chain_window: an as-written deletion links to an energy-only creation row of its type");
        if (lk == -2 && k != MGPU_CREATION) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: energy-only rows are creation-kind");
        const int mc = (k == MGPU_CREATION) ? -1 : m[c];
        if ((rc = check_candidate(e, c, replica, t[c], mc, k != MGPU_CREATION))) return rc;
        if (k == MGPU_CREATION && lk != -2 && e->h_nmol[idx] >= e->tp.cap[t[c]])
            return set_error(MGPU_ERR_CAPACITY, "chain_window: residue type is at mol_capacity");
        if (!wide_row) k_rows = std::max(k_rows, e->win.k_lds[t[c]]);
        g.t[c] = t[c]; g.m[c] = mc; g.kind[c] = (signed char)k; g.link[c] = (signed char)lk;
        g.u[c] = accept_u[c]; g.pref[c] = accept_pref[c];
        const double *row = sites + (size_t)c * site_stride * 3;
        cand_ok[c] = 1;
        if (k != MGPU_DELETION) {
            // the engine's site order for a frozen type is not the caller's: such types are inactive and never move
            if (e->frozen[t[c]]) return set_error(MGPU_ERR_INVALID_ARG, "chain_window: frozen residue types do not move");
            std::memcpy(wide_row ? wide_rows + (size_t)c * kFarmWideSites * 3 : &g.sites[c][0][0], row, (size_t)n1 * 3 * sizeof(double));
            cand_ok[c] = sites_in_range(e, row, n1) ? 1 : 0;
            if (lk != -2) fast = fast && cand_ok[c];
        }
        g.ent_old_of[c] = g.ent_new_of[c] = -1;
        if (lk == -2) continue;
        if (k != MGPU_CREATION) { g.ent_old_of[c] = (signed char)n_ent; g.ent_c[n_ent] = (unsigned char)c; g.ent_new[n_ent] = 0; ++n_ent; }
        if (k != MGPU_DELETION) { g.ent_new_of[c] = (signed char)n_ent; g.ent_c[n_ent] = (unsigned char)c; g.ent_new[n_ent] = 1; ++n_ent; }
    }
    const int nsplit = e->pair_nsplit;
    // a row of more than kMaxFusedSitesWide sites: the WIDE instance, else the narrow one
    const size_t lds = window_lds(e, kPathChain, wide, k_rows, n_ent);
    if (!window_lds_fits(wide, lds)) return set_error(MGPU_ERR_CAPACITY, "chain_window: the window does not fit the LDS budget");
    auto wide_family = [](auto &&f, auto FLAT, auto FASTW) { f(chain_window_kernel<decltype(FLAT)::value, decltype(FASTW)::value, false, true>); };
    auto tri_wide_family = [](auto &&f) { f(chain_window_kernel<false, false, true, true>); };
    if ((rc = lds_opt_in(e->device, kLdsChainWide, lds, [&](auto &&f) {
             for_all_bools([&](auto... flags) { wide_family(f, flags...); }, std::integral_constant<int, 2>{});
             tri_wide_family(f);
         })))
        return rc;
    ch.seq += 1;
    for (int tt = 0; tt < e->tp.n_res; ++tt) g.self_of_type[tt] = e->self_of_type[tt];
    g.stamps = ch.timing ? 1 : 0;
    g.res = ch.d_res; g.partials = ch.d_part; g.ticket = ch.d_ticket; g.alt = ch.d_alt;
    g.host_out = ch.h_out; g.host_tag = ch.h_tag; g.seq = ch.seq;
    g.n = n; g.n_ent = n_ent; g.nsplit = nsplit; g.replica = replica;
    g.temperature = temperature; g.e_recip = recip_energy; g.margin = ch.margin;
    if (wide) {
        g.wide_sites = wide_rows;
        wide_args(e, &g.row_first, &g.wide_at, g.kform, g.wide_rpt, g.wide_nss);
    }
    const int grid = n + (n_ent * nsplit + kPairWaves - 1) / kPairWaves;
    const bool ff = fast && e->pair_fast_fold;
    ln.dirty = true;
    ln.forget_trial();
    auto launch = [&](auto kernel) { window_launch(kernel, e, d_topo, grid, lds, ln.stream, g); };
    // (the image search has no flat and no fast-fold form; a WIDE row of a triclinic box got here under mgpu_chain_set_wide_triclinic)
    if (e->bx.triclinic && wide) tri_wide_family(launch);
    else if (e->bx.triclinic) launch(chain_window_kernel<false, false, true>);
    else if (wide) with_bools([&](auto... flags) { wide_family(launch, flags...); }, e->pair_flat, ff);
    else with_bools([&](auto FLAT, auto FASTW) { launch(chain_window_kernel<decltype(FLAT)::value, decltype(FASTW)::value>); }, e->pair_flat, ff);
    HIP_TRY(hipGetLastError());
    // ---- wait for the tag: the results are in host memory when it shows this window's number
    if ((rc = wait_for_tag(ln.stream, ch.h_tag, 1, ch.seq, 20000, 4096, "chain_window"))) return rc;
    for (int c = 0; c < n; ++c) copy_energy_rows(old_energy, new_energy, c, ch.h_out + 10 * (size_t)c);
    const int *hi = (const int *)(ch.h_out + 10 * (size_t)kChainMaxCand);
    const int first = hi[0], und = hi[1];
    *first_accepted = first;
    *undecided = und;
    ch.windows += 1;
    if (und >= 0) ch.undecided += 1;
    if (first >= 0) mirror_accepted(e, replica, t[first], kind[first], cand_ok[first] != 0);
    return MGPU_OK;
}


// ---- farm windows ------------------------------------------------------------------------------
// One launch per lane step of a farm of chains (farm_window_kernel, mgpu_kernels_windows.h): the caller hands over, per chain, the
// move it selected and the uniform numbers of its construction and of its acceptance test; the launch evaluates,
// decides and commits; the host collects energies and verdicts from pinned memory by polling per-chain tags.  Up to
// kFarmDepth windows per lane may be in flight (a farm whose move selection does not depend on earlier outcomes -- NVT --
// queues the next step before it has seen the last).

int mgpu_farm_window_capacity(const mgpu_engine *e, int *max_chains, int *max_in_flight) {
    if (!e || !max_chains) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_capacity: null argument");
    *max_chains = window_admission(e, kPathFarm).capacity;
    if (max_in_flight) *max_in_flight = kFarmDepth;
    return MGPU_OK;
}

int mgpu_farm_set_wide_triclinic(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    // every refusal leaves the switch as it was
    if (!e->bx.triclinic) return set_error(MGPU_ERR_STATE, "farm_set_wide_triclinic: the box is orthorhombic");
    int rc = use_device(e);
    if (rc) return rc;
    // (a window in flight was admitted, and its LDS sized, under the switch as it stands: it is collected first)
    if (!on)
        for (int l = 0; l < kLanes; ++l)
            if (!e->lanes[l].farm.pending.empty())
                return set_error(MGPU_ERR_STATE, "farm_set_wide_triclinic: a farm window is in flight (mgpu_farm_window_wait)");
    if ((rc = sync_all_lanes(e))) return rc;      // (no trial or window in flight sees the switch move)
    e->farm_wide_tri = on != 0;
    return MGPU_OK;
}

int mgpu_farm_window_get_stats(const mgpu_engine *e, long long *windows, long long *undecided) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (windows) *windows = e->farm.windows;
    if (undecided) *undecided = e->farm.undecided;
    return MGPU_OK;
}

static int farm_lane(mgpu_engine *e, int lane, Lane **ln) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    if (lane < 0 || lane >= kLanes) return set_error(MGPU_ERR_INVALID_ARG, "lane out of range");
    *ln = &e->lanes[lane];
    return MGPU_OK;
}

// the lane's blocks for windows of up to `cap` chains; the engine's second A(k) buffer and flags
static int farm_reserve(mgpu_engine *e, Lane &ln, int cap) {
    Lane::FarmWindow &fw = ln.farm;
    if (int rc = alt_reserve(e)) return rc;
    if (!e->farm.d_stalled) {
        HIP_TRY(hipMalloc((void **)&e->farm.d_stalled, (size_t)e->n_replicas * sizeof(int)));
        HIP_TRY(hipMemset(e->farm.d_stalled, 0, (size_t)e->n_replicas * sizeof(int)));
        HIP_TRY(hipDeviceSynchronize());
    }
    if (cap <= fw.cap) return MGPU_OK;
    if (!fw.pending.empty()) return set_error(MGPU_ERR_STATE, "farm_window_submit: a larger window than the lane's blocks while windows are in flight");
    HIP_TRY(hipStreamSynchronize(ln.stream));
    const unsigned long long seq = fw.seq;
    fw.release();
    fw.seq = seq;
    cap = std::max(cap, 64);
    HIP_TRY(hipHostMalloc((void **)&fw.h_recs, (size_t)kFarmDepth * cap * sizeof(FarmRec), hipHostMallocCoherent));
    HIP_TRY(hipHostMalloc((void **)&fw.h_out, (size_t)kFarmDepth * cap * kFarmOut * sizeof(double), hipHostMallocCoherent));
    HIP_TRY(hipHostMalloc((void **)&fw.h_tag, (size_t)kFarmDepth * cap * sizeof(unsigned long long), hipHostMallocCoherent));
    std::memset(fw.h_tag, 0xff, (size_t)kFarmDepth * cap * sizeof(unsigned long long));      // no window carries this number
    HIP_TRY(hipMalloc((void **)&fw.d_part, (size_t)cap * 2 * e->pair_nsplit * sizeof(double2)));
    HIP_TRY(hipMalloc((void **)&fw.d_res, (size_t)cap * sizeof(ChainResult)));
    HIP_TRY(hipMalloc((void **)&fw.d_tickets, (size_t)cap * sizeof(int)));
    HIP_TRY(hipMemset(fw.d_tickets, 0, (size_t)cap * sizeof(int)));
    HIP_TRY(hipMemset(fw.d_res, 0, (size_t)cap * sizeof(ChainResult)));
    HIP_TRY(hipDeviceSynchronize());
    fw.cap = cap;
    return MGPU_OK;
}

int mgpu_farm_window_submit(mgpu_engine *e, int lane, int n, const int *replica, const int *t, const int *m, const int *move,
                            const int *forced, const double *u5, const double *accept_u, const double *accept_pref,
                            const double *slot_u, double t_step, double r_step, double temperature) {
    Lane *lp = nullptr;
    int rc = farm_lane(e, lane, &lp);
    if (rc) return rc;
    Lane &ln = *lp;
    if (!replica || !t || !m || !move || !u5 || !accept_u || !accept_pref)
        return set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: null argument");
    const WindowAdmission adm = window_admission(e, kPathFarm);
    const int n_max = adm.capacity;
    if (n_max == 0) return set_error(MGPU_ERR_STATE, "farm_window_submit: not available for this engine (mgpu_farm_window_capacity)");
    if (n < 1 || n > n_max) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: number of chains out of range");
    if (!(temperature > 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: temperature must be positive");
    if ((rc = use_device(e))) return rc;
    if (ln.n_submitted != 0) return set_error(MGPU_ERR_STATE, "farm_window_submit: the lane still holds an un-waited trial");
    Lane::FarmWindow &fw = ln.farm;
    if ((int)fw.pending.size() >= kFarmDepth) return set_error(MGPU_ERR_STATE, "farm_window_submit: too many windows of this lane in flight");
    if (!fw.pending.empty() && fw.pending.back().counts_change)
        return set_error(MGPU_ERR_STATE, "farm_window_submit: the lane's last window carries an insertion / deletion: collect it first");
    const Topo *d_topo = nullptr;
    {
        // (one lane at a time: the engine's second A(k) buffer, its flags and the device topology are made on first use)
        std::lock_guard<std::mutex> lock(e->farm.mu);
        if ((rc = farm_reserve(e, ln, n))) return rc;
        if ((rc = chain_topo(e, &d_topo))) return rc;
    }
    const int slot = (int)(fw.seq % kFarmDepth);
    Lane::FarmWindow::Pending pd;
    pd.seq = fw.seq + 1;
    pd.n = n; pd.slot = slot; pd.counts_change = false;
    pd.rep.assign(replica, replica + n);
    pd.t.assign(t, t + n);
    pd.kind.assign(n, -1);
    pd.ok.assign(n, 1);
    FarmArgs g{};
    FarmRec *recs = n <= kFarmInline ? g.inline_recs : fw.h_recs + (size_t)slot * fw.cap;
    bool fast = true, wide = false;
    size_t k_rows = 0;
    std::string why;
    for (int c = 0; c < n; ++c) {
        FarmRec &r = recs[c];
        r = FarmRec{};
        const int mv = move[c];
        if (mv < 0 || mv > 4) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: unknown move code"); break; }
        if (replica[c] < 0 || replica[c] >= e->n_replicas) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: replica out of range"); break; }
        r.replica = replica[c];
        if (mv == 0) continue;                                   // the chain does nothing this step
        if (t[c] < 0 || t[c] >= e->tp.n_res) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: residue type out of range"); break; }
        if (!adm.rides[t[c]]) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: molecule too large for the one-launch path"); break; }
        const size_t idx = (size_t)replica[c] * e->tp.n_res + t[c];
        const int k = mv <= 2 ? MGPU_MOVE : (mv == 3 ? MGPU_CREATION : MGPU_DELETION);
        if ((rc = admit_built(e, idx, k, mv, kAdmitFrames, "farm_window_submit", "chain", c, why, pd.ok[c], fast))) { set_error(rc, why); break; }
        const int mc = k == MGPU_CREATION ? -1 : (slot_u ? 0 : m[c]);
        if (!slot_u) {
            // the caller picked the molecule: against the engine's counts, which must then be current
            if ((rc = check_candidate(e, c, replica[c], t[c], mc, k != MGPU_CREATION))) break;
            if (k == MGPU_CREATION && e->h_nmol[idx] >= e->tp.cap[t[c]]) { rc = set_error(MGPU_ERR_CAPACITY, "farm_window_submit: residue type is at mol_capacity"); break; }
            if (k != MGPU_MOVE) pd.counts_change = true;
        } else {
            // the device picks it from the replica's count when the launch runs (FarmRec::by_count)
            if (!(slot_u[c] >= 0.0 && slot_u[c] < 1.0)) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: slot_u must lie in [0, 1)"); break; }
            r.by_count = 1;
            r.sel_u = slot_u[c];
        }
        fast = fast && replica_in_range(e, replica[c]);
        if ((rc = admit_built(e, idx, k, mv, kAdmitInsertion | kAdmitRange, "farm_window_submit", "chain", c, why, pd.ok[c], fast))) { set_error(rc, why); break; }
        wide = wide || window_takes_wide(e, kPathFarm, t[c]);
        k_rows = std::max(k_rows, e->win.k_lds[t[c]]);
        pd.kind[c] = k;
        // windows still in flight behind this one must not take the fast fold if this step is accepted: the range flag is
        // lowered now, not when the window is collected (a rejected step costs the replica the fast fold and nothing else)
        if (k != MGPU_DELETION && !pd.ok[c]) e->in_range[idx] = 0;
        r.t = t[c]; r.m = (k == MGPU_CREATION || slot_u) ? 0 : m[c]; r.move = mv;
        r.forced = forced ? forced[c] : 0;
        if (r.forced < 0 || r.forced > 2) { rc = set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: forced is 0, 1 (accept) or 2 (reject)"); break; }
        for (int d = 0; d < 5; ++d) r.u[d] = u5[5 * (size_t)c + d];
        r.acc_u = accept_u[c];
        r.pref = accept_pref[c];
    }
    if (rc) return rc;
    if (!one_record_per_replica(ln, e->n_replicas, replica, n)) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_submit: more than one chain record for a replica");
    if (pd.counts_change && !fw.pending.empty())
        return set_error(MGPU_ERR_STATE, "farm_window_submit: a window with an insertion / deletion needs the lane's earlier windows collected "
                                         "(its molecule counts must be current)");
    const int nsplit = e->pair_nsplit;
    // a chain of more than kMaxFusedSitesWide sites: the WIDE instance, else the narrow one
    const size_t lds = window_lds(e, kPathFarm, wide, k_rows, n);
    if (!window_lds_fits(wide, lds)) return set_error(MGPU_ERR_CAPACITY, "farm_window_submit: the window does not fit the LDS budget");
    // The window kernel's families: with the image search (no flat form, no fast fold; a WIDE chain of such a box got here under
    // mgpu_farm_set_wide_triclinic), WIDE, narrow; within each the flags are free.  (An engine without reservoirs runs the
    // instances without their code.)
    auto tri_family = [](auto &&f, auto WIDE, auto RSV) {
        f(farm_window_kernel<false, false, decltype(WIDE)::value, decltype(RSV)::value, true>);
    };
    auto wide_family = [](auto &&f, auto FLAT, auto FASTW, auto RSV) {
        f(farm_window_kernel<decltype(FLAT)::value, decltype(FASTW)::value, true, decltype(RSV)::value>);
    };
    auto narrow_family = [](auto &&f, auto FLAT, auto FASTW, auto RSV) {
        f(farm_window_kernel<decltype(FLAT)::value, decltype(FASTW)::value, false, decltype(RSV)::value>);
    };
    if ((rc = lds_opt_in(e->device, kLdsFarmWide, lds, [&](auto &&f) {
             for_all_bools([&](auto... flags) { wide_family(f, flags...); }, std::integral_constant<int, 3>{});
             for_all_bools([&](auto RSV) { tri_family(f, std::true_type{}, RSV); }, std::integral_constant<int, 1>{});
         })))
        return rc;
    fw.seq += 1;
    for (int tt = 0; tt < e->tp.n_res; ++tt) g.self_of_type[tt] = e->self_of_type[tt];
    g.recs = fw.h_recs + (size_t)slot * fw.cap;
    g.partials = fw.d_part; g.res = fw.d_res; g.tickets = fw.d_tickets;
    g.stalled = e->farm.d_stalled; g.acur = e->d_acur; g.A_alt = e->d_A_alt;
    g.host_out = fw.h_out + (size_t)slot * fw.cap * kFarmOut;
    g.host_tag = fw.h_tag + (size_t)slot * fw.cap;
    g.seq = pd.seq;
    g.n = n; g.nsplit = nsplit;
    g.t_step = t_step; g.r_step = r_step; g.temperature = temperature; g.margin = e->chain.margin;
    if (wide) {
        wide_args(e, &g.row_first, &g.wide_at, g.kform, g.wide_rpt, g.wide_nss);
    }
    const int wpc = 2 * nsplit;
    const int grid = (n * wpc + kPairWaves - 1) / kPairWaves + n;
    const bool ff = fast && e->pair_fast_fold;
    ln.dirty = true;
    ln.forget_trial();
    for (int c = 0; c < n; ++c) alt_forget(e, replica[c]);     // (the window's k role overwrites their other buffers)
    e->a_switched = true;
    auto launch = [&](auto kernel) { window_launch(kernel, e, d_topo, grid, lds, ln.stream, g); };
    if (e->bx.triclinic) with_bools([&](auto... flags) { tri_family(launch, flags...); }, wide, e->rsv_any);
    else if (wide) with_bools([&](auto... flags) { wide_family(launch, flags...); }, e->pair_flat, ff, e->rsv_any);
    else with_bools([&](auto... flags) { narrow_family(launch, flags...); }, e->pair_flat, ff, e->rsv_any);
    HIP_TRY(hipGetLastError());
    fw.pending.push_back(std::move(pd));
    e->farm.windows += 1;
    return MGPU_OK;
}

// The lane's OLDEST window in flight: energies (rows of five: non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb,
// as mgpu_gcmc_trial_wait fills them) and one verdict per chain -- 0 rejected, 1 accepted (and committed), 2 undecided (the
// host decides and sends the step again with `forced`), 4 nothing done: the replica waits for such a decision, 5 idle record.
int mgpu_farm_window_wait(mgpu_engine *e, int lane, double *old_energy, double *new_energy, int *verdict) {
    Lane *lp = nullptr;
    int rc = farm_lane(e, lane, &lp);
    if (rc) return rc;
    Lane &ln = *lp;
    if (!old_energy || !new_energy || !verdict) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_wait: null argument");
    Lane::FarmWindow &fw = ln.farm;
    if (fw.pending.empty()) return set_error(MGPU_ERR_STATE, "farm_window_wait: no window of this lane is in flight");
    const Lane::FarmWindow::Pending &pd = fw.pending.front();
    const int n = pd.n;
    const double *out = fw.h_out + (size_t)pd.slot * fw.cap * kFarmOut;
    // (a window lost either way leaves the queue, so that the lane is not left waiting for it)
    if ((rc = wait_for_tag(ln.stream, fw.h_tag + (size_t)pd.slot * fw.cap, n, pd.seq, 200000, 65536, "farm_window_wait"))) {
        fw.pending.pop_front();
        return rc;
    }
    for (int c = 0; c < n; ++c) {
        const double *o = out + (size_t)kFarmOut * c;
        copy_energy_rows(old_energy, new_energy, c, o);
        const int v = (int)o[10];
        verdict[c] = v;
        if (v == kFarmVerdictUndecided) e->farm.undecided += 1;
        if (v != kFarmVerdictAccepted) continue;
        mirror_accepted(e, pd.rep[c], pd.t[c], pd.kind[c], true);   // (the range flag was lowered at submit)
    }
    fw.pending.pop_front();
    return MGPU_OK;
}

// ---- chain runs --------------------------------------------------------------------------------
// Launches of ONE chain queued back to back on lane 0, each continuing from the cursor in device memory (chain_run_kernel,
// mgpu_kernels_windows.h).  Host state (e->run) is touched by the run's one driver thread only.

// the tags of the launches that have finished since the last look, in order: counters and the launch log
static void run_poll(mgpu_engine *e) {
    mgpu_engine::Run &rn = e->run;
    const volatile unsigned long long *info = rn.h_launch, *tag = rn.h_launch + kRunLaunchRing;
    while (rn.seq_done < rn.seq) {
        const unsigned long long s = rn.seq_done + 1;
        if (tag[s % kRunLaunchRing] != s) break;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const unsigned long long v = info[s % kRunLaunchRing];
        const int first = (int)(v >> 16), consumed = (int)((v >> 8) & 0xff), flags = (int)(v & 0xff);
        rn.launches += 1;
        rn.steps += consumed;
        if (flags & kRunTagVoid) rn.void_launches += 1;
        else if (flags & kRunTagStalled) rn.undecided += 1;
        rn.dev_stalled = (flags & kRunTagStalled) != 0;
        rn.log.emplace_back(first, consumed);
        if ((int)rn.log.size() > kRunLogMax) rn.log.pop_front();
        rn.seq_done = s;
    }
}

// a decided step has been read: the host's counts follow an accepted insertion / deletion (once per step, in order)
static void run_mirror(mgpu_engine *e, long long step) {
    mgpu_engine::Run &rn = e->run;
    if (step < rn.mirrored) return;
    rn.mirrored = step + 1;
    const RunRec &r = rn.h_ring[step % kRunRingSteps];
    if (r.move < 3 || (int)rn.h_out[(size_t)(step % kRunRingSteps) * kRunOut + 10] != kFarmVerdictAccepted) return;
    mirror_accepted(e, rn.replica, r.t, r.move == 3 ? MGPU_CREATION : MGPU_DELETION, true);   // (the range flag was lowered at the push)
}

static int run_launch_one(mgpu_engine *e, int force_step, int force_verdict) {
    mgpu_engine::Run &rn = e->run;
    Lane &ln = e->lanes[0];
    const Topo *d_topo = nullptr;
    int rc = chain_topo(e, &d_topo);
    if (rc) return rc;
    const int nsplit = e->pair_nsplit;
    size_t k_rows = 0;
    for (int t = 0; t < e->tp.n_res; ++t)
        if (e->is_active[t]) k_rows = std::max(k_rows, e->win.k_lds[t]);
    // the WIDE instances when any active type has more than kMaxFusedSitesWide sites: the run's choice, not the launch's (which
    // records a launch consumes is known on the device alone)
    bool wide = false;
    for (int t = 0; t < e->tp.n_res; ++t) wide = wide || (e->is_active[t] && window_takes_wide(e, kPathRun, t));
    const size_t lds = window_lds(e, kPathRun, wide, k_rows, rn.k);
    if (!window_lds_fits(wide, lds)) return set_error(MGPU_ERR_CAPACITY, "chain_run_launch: the launch does not fit the LDS budget");
    auto wide_family = [](auto &&f, auto FLAT, auto FASTW, auto GC) {
        f(chain_run_kernel<decltype(FLAT)::value, decltype(FASTW)::value, false, decltype(GC)::value, true>);
    };
    auto tri_wide_family = [](auto &&f, auto GC) { f(chain_run_kernel<false, false, true, decltype(GC)::value, true>); };
    if (wide && (rc = lds_opt_in(e->device, kLdsRunWide, lds, [&](auto &&f) {
             for_all_bools([&](auto... flags) { wide_family(f, flags...); }, std::integral_constant<int, 3>{});
             for_all_bools([&](auto... flags) { tri_wide_family(f, flags...); }, std::integral_constant<int, 1>{});
         })))
        return rc;
    ChainRunArgs g{};
    rn.seq += 1;
    g.state = rn.d_state; g.ring = rn.d_ring; g.partials = rn.d_part; g.res = rn.d_res; g.ticket = rn.d_ticket; g.alt = rn.d_alt;
    g.host_out = rn.h_out; g.step_tag = rn.h_step_tag;
    g.launch_info = rn.h_launch + rn.seq % kRunLaunchRing;
    g.launch_tag = rn.h_launch + kRunLaunchRing + rn.seq % kRunLaunchRing;
    g.seq = rn.seq;
    g.k = rn.k; g.nsplit = nsplit; g.replica = rn.replica; g.ring_steps = kRunRingSteps;
    g.force_step = force_step; g.force_verdict = force_verdict;
    g.t_step = rn.t_step; g.r_step = rn.r_step; g.temperature = rn.temperature; g.margin = e->chain.margin;
    if (rn.gc) {
        g.gc_ring = rn.d_gc;
        for (int tt = 0; tt < e->tp.n_res; ++tt) g.self_of_type[tt] = e->self_of_type[tt];
    }
    if (wide) wide_args(e, &g.row_first, &g.wide_at, g.kform, g.wide_rpt, g.wide_nss);
    const int grid = (rn.k * 2 * nsplit + kPairWaves - 1) / kPairWaves + rn.k;
    const bool ff = rn.fast && e->pair_fast_fold;
    ln.dirty = true;
    ln.forget_trial();
    alt_forget(e, rn.replica);
    // The run kernel's families: with the image search (no flat form, no fast fold: farm_window_kernel's triclinic family), the
    // orthorhombic one, whose flags are free, and the grand-canonical forms of both (the run was opened with the switch on); the
    // WIDE families above (orthorhombic, and with the image search under mgpu_chain_set_wide_triclinic; NVT and grand-canonical)
    // for an engine with an active type of 6..63 sites.
    auto tri_family = [](auto &&f) { f(chain_run_kernel<false, false, true>); };
    auto ortho_family = [](auto &&f, auto FLAT, auto FASTW) { f(chain_run_kernel<decltype(FLAT)::value, decltype(FASTW)::value>); };
    auto gc_family = [](auto &&f, auto FLAT, auto FASTW) { f(chain_run_kernel<decltype(FLAT)::value, decltype(FASTW)::value, false, true>); };
    auto tri_gc_family = [](auto &&f) { f(chain_run_kernel<false, false, true, true>); };
    auto launch = [&](auto kernel) { window_launch(kernel, e, d_topo, grid, lds, ln.stream, g); };
    if (e->bx.triclinic && wide) with_bools([&](auto... flags) { tri_wide_family(launch, flags...); }, rn.gc);
    else if (e->bx.triclinic && rn.gc) tri_gc_family(launch);
    else if (e->bx.triclinic) tri_family(launch);
    else if (wide) with_bools([&](auto... flags) { wide_family(launch, flags...); }, e->pair_flat, ff, rn.gc);
    else if (rn.gc) with_bools([&](auto... flags) { gc_family(launch, flags...); }, e->pair_flat, ff);
    else with_bools([&](auto... flags) { ortho_family(launch, flags...); }, e->pair_flat, ff);
    HIP_TRY(hipGetLastError());
    return MGPU_OK;
}

int mgpu_chain_run_capacity(const mgpu_engine *e, int *max_k, int *max_in_flight, int *ring_steps) {
    if (!e || !max_k) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_capacity: null argument");
    const int k = window_admission(e, kPathRun).capacity;
    *max_k = k;
    if (max_in_flight) *max_in_flight = k ? kRunMaxInFlight : 0;
    if (ring_steps) *ring_steps = k ? kRunRingSteps : 0;
    return MGPU_OK;
}

int mgpu_chain_run_set_triclinic(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    // every refusal leaves the switch as it was
    if (!e->bx.triclinic) return set_error(MGPU_ERR_STATE, "chain_run_set_triclinic: the box is orthorhombic");
    if (!e->tri_moves) return set_error(MGPU_ERR_STATE, "chain_run_set_triclinic: device-built triclinic moves are off (mgpu_set_triclinic_moves)");
    if (e->run.open) return set_error(MGPU_ERR_STATE, "chain_run_set_triclinic: a run is open");
    // (grand-canonical runs of a triclinic box stand on this switch: mgpu_chain_run_set_gc)
    if (!on && e->run.gc) return set_error(MGPU_ERR_STATE, "chain_run_set_triclinic: grand-canonical runs are on (mgpu_chain_run_set_gc)");
    e->run.triclinic = on != 0;
    return MGPU_OK;
}

int mgpu_chain_run_set_wide(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    // every refusal leaves the switch as it was
    if (e->run.open) return set_error(MGPU_ERR_STATE, "chain_run_set_wide: a run is open");
    if (on && e->bx.triclinic && !e->wide_tri)
        return set_error(MGPU_ERR_STATE, "chain_run_set_wide: the box is triclinic (no WIDE sweep has the image search unless "
                                         "mgpu_chain_set_wide_triclinic is on)");
    if (on && e->rsv_any) return set_error(MGPU_ERR_STATE, "chain_run_set_wide: the engine holds a reservoir (no RSV instance of the run kernel)");
    e->run.wide = on != 0;
    return MGPU_OK;
}

int mgpu_chain_run_set_gc(mgpu_engine *e, int on) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    // every refusal leaves the switch as it was
    if (on && e->bx.triclinic && !e->run.triclinic)
        return set_error(MGPU_ERR_STATE, "chain_run_set_gc: the box is triclinic and triclinic runs are off (mgpu_chain_run_set_triclinic)");
    if (e->rsv_any) return set_error(MGPU_ERR_STATE, "chain_run_set_gc: the engine holds a reservoir (no such instance of the run kernel)");
    if (e->run.open) return set_error(MGPU_ERR_STATE, "chain_run_set_gc: a run is open");
    e->run.gc = on != 0;
    return MGPU_OK;
}

int mgpu_chain_run_open(mgpu_engine *e, int replica, int k, double t_step, double r_step, double temperature) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    const int k_max = window_admission(e, kPathRun).capacity;
    if (k_max == 0) return set_error(MGPU_ERR_STATE, "chain_run_open: not available for this engine (mgpu_chain_run_capacity)");
    if (rn.open) return set_error(MGPU_ERR_STATE, "chain_run_open: a run is open (one per engine)");
    if (replica < 0 || replica >= e->n_replicas) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_open: replica out of range");
    if (k < 1 || k > k_max) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_open: steps per launch out of range");
    if (!(temperature > 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_open: temperature must be positive");
    for (int t = 0; t < e->tp.n_res; ++t)
        if (e->is_active[t] && (!e->d_com || !e->frames_ok[(size_t)replica * e->tp.n_res + t]))
            return set_error(MGPU_ERR_STATE, "chain_run_open: no molecule frames for this replica (mgpu_replica_set_frames)");
    int rc = use_device(e);
    if (rc) return rc;
    Lane &ln = e->lanes[0];
    if (ln.n_submitted != 0 || !ln.farm.pending.empty())
        return set_error(MGPU_ERR_STATE, "chain_run_open: lane 0 still holds an un-waited trial or farm window");
    if ((rc = sync_all_lanes(e))) return rc;                    // (every replica's A(k) in its primary buffer: the run reads and writes d_A)
    if (!rn.d_state) {
        HIP_TRY(hipMalloc((void **)&rn.d_state, sizeof(RunState)));
        HIP_TRY(hipMalloc((void **)&rn.d_ring, sizeof(RunRec) * kRunRingSteps));
        HIP_TRY(hipHostMalloc((void **)&rn.h_ring, sizeof(RunRec) * kRunRingSteps, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&rn.h_pushed, sizeof(int) * kRunRingSteps, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&rn.h_out, sizeof(double) * kRunOut * kRunRingSteps, hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc((void **)&rn.h_step_tag, sizeof(unsigned long long) * kRunRingSteps, hipHostMallocCoherent));
        HIP_TRY(hipHostMalloc((void **)&rn.h_launch, sizeof(unsigned long long) * 2 * kRunLaunchRing, hipHostMallocCoherent));
        std::memset(rn.h_launch, 0, sizeof(unsigned long long) * 2 * kRunLaunchRing);
        HIP_TRY(hipMalloc((void **)&rn.d_part, sizeof(double2) * 2 * kRunMaxK * (size_t)e->pair_nsplit));
        HIP_TRY(hipMalloc((void **)&rn.d_res, sizeof(ChainResult) * kRunMaxK));
        HIP_TRY(hipMalloc((void **)&rn.d_alt, sizeof(double2) * kRunMaxK * (size_t)e->n_slots));
        HIP_TRY(hipMalloc((void **)&rn.d_ticket, sizeof(int)));
        HIP_TRY(hipMemset(rn.d_ticket, 0, sizeof(int)));
    }
    if (rn.gc && !rn.d_gc) {
        HIP_TRY(hipMalloc((void **)&rn.d_gc, sizeof(double2) * kRunRingSteps));
        HIP_TRY(hipHostMalloc((void **)&rn.h_gc, sizeof(double2) * kRunRingSteps, hipHostMallocDefault));
    }
    const Topo *d_topo = nullptr;
    if ((rc = chain_topo(e, &d_topo))) return rc;
    HIP_TRY(hipMemset(rn.d_state, 0, sizeof(RunState)));
    HIP_TRY(hipDeviceSynchronize());
    std::memset(rn.h_step_tag, 0, sizeof(unsigned long long) * kRunRingSteps);
    rn.open = true;
    rn.replica = replica; rn.k = k;
    rn.t_step = t_step; rn.r_step = r_step; rn.temperature = temperature;
    rn.fast = replica_in_range(e, replica);
    rn.pushed = rn.collected = rn.mirrored = 0;
    rn.stalled_at = -1;
    rn.dev_stalled = false;
    rn.seq_done = rn.seq;
    rn.log.clear();
    return MGPU_OK;
}

// the records [pushed, pushed + n) of the ring's image (a slot is rewritten only after its step has been collected) to the
// device, then the count, on the launches' stream and ahead of the launches that read them
static int run_push_copy(mgpu_engine *e, int n, bool gc) {
    mgpu_engine::Run &rn = e->run;
    Lane &ln = e->lanes[0];
    ln.dirty = true;
    const int s0 = (int)(rn.pushed % kRunRingSteps), n0 = std::min(n, kRunRingSteps - s0);
    HIP_TRY(hipMemcpyAsync(rn.d_ring + s0, rn.h_ring + s0, sizeof(RunRec) * n0, hipMemcpyHostToDevice, ln.stream));
    if (n > n0) HIP_TRY(hipMemcpyAsync(rn.d_ring, rn.h_ring, sizeof(RunRec) * (n - n0), hipMemcpyHostToDevice, ln.stream));
    if (gc) {
        HIP_TRY(hipMemcpyAsync(rn.d_gc + s0, rn.h_gc + s0, sizeof(double2) * n0, hipMemcpyHostToDevice, ln.stream));
        if (n > n0) HIP_TRY(hipMemcpyAsync(rn.d_gc, rn.h_gc, sizeof(double2) * (n - n0), hipMemcpyHostToDevice, ln.stream));
    }
    rn.pushed += n;
    int *cnt = rn.h_pushed + rn.pushed % kRunRingSteps;
    *cnt = (int)rn.pushed;
    HIP_TRY(hipMemcpyAsync(&rn.d_state->pushed, cnt, sizeof(int), hipMemcpyHostToDevice, ln.stream));
    return MGPU_OK;
}

int mgpu_chain_run_push(mgpu_engine *e, int n, const int *t, const int *m, const int *move, const double *u5, const double *accept_u) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_push: no run is open");
    if (n < 0 || (n > 0 && (!t || !m || !move || !u5 || !accept_u))) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: bad argument");
    if (n == 0) return MGPU_OK;
    if (rn.pushed + n - rn.collected > kRunRingSteps)
        return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: beyond the ring (steps pushed and not yet collected: mgpu_chain_run_capacity)");
    if (rn.pushed + n >= (1ll << 30)) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: too many steps in one run");
    int rc = use_device(e);
    if (rc) return rc;
    // every record is checked before any is written: a refused push leaves the run as it was
    bool fast = rn.fast;
    const WindowAdmission adm = window_admission(e, kPathRun);
    for (int c = 0; c < n; ++c) {
        const int mv = move[c];
        if (mv == 3 || mv == 4) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: insertions and deletions do not ride in a run (moves only)");
        if (mv < 0 || mv > 4) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: unknown move code");
        if (mv == 0) continue;
        if (t[c] < 0 || t[c] >= e->tp.n_res || !adm.rides[t[c]])
            return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push: residue type out of range or not active");
        if ((rc = check_candidate(e, c, rn.replica, t[c], m[c], true))) return rc;
        fast = fast && e->frames_tight[(size_t)rn.replica * e->tp.n_res + t[c]];
    }
    for (int c = 0; c < n; ++c) {
        RunRec &r = rn.h_ring[(rn.pushed + c) % kRunRingSteps];
        r = RunRec{};
        r.move = move[c];
        if (r.move == 0) continue;
        r.t = t[c]; r.m = m[c];
        for (int d = 0; d < 5; ++d) r.u[d] = u5[5 * (size_t)c + d];
        r.acc_u = accept_u[c];
        // a step that is accepted may leave the fast fold's range: the flag is lowered now (mgpu_farm_window_submit's rule)
        const size_t idx = (size_t)rn.replica * e->tp.n_res + t[c];
        if (!e->frames_tight[idx]) e->in_range[idx] = 0;
    }
    rn.fast = fast;
    return run_push_copy(e, n, false);
}

// By-count records of a grand-canonical run (mgpu_chain_run_set_gc): the device picks the molecule and forms the prefactor from
// the count each launch finds (chain_run_kernel<..., GC>), so no slot is given and none is checked against the host's counts.
int mgpu_chain_run_push_gc(mgpu_engine *e, int n, const int *t, const int *move, const double *u5, const double *accept_u,
                           const double *sel_u, const double *phi_v) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_push_gc: no run is open");
    if (!rn.gc) return set_error(MGPU_ERR_STATE, "chain_run_push_gc: grand-canonical runs are off (mgpu_chain_run_set_gc)");
    if (n < 0 || (n > 0 && (!t || !move || !u5 || !accept_u || !sel_u || !phi_v)))
        return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: bad argument");
    if (n == 0) return MGPU_OK;
    if (rn.pushed + n - rn.collected > kRunRingSteps)
        return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: beyond the ring (steps pushed and not yet collected: mgpu_chain_run_capacity)");
    if (rn.pushed + n >= (1ll << 30)) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: too many steps in one run");
    int rc = use_device(e);
    if (rc) return rc;
    // every record is checked before any is written: a refused push leaves the run as it was
    bool fast = rn.fast;
    const WindowAdmission adm = window_admission(e, kPathRun);
    std::string why;
    for (int c = 0; c < n; ++c) {
        const int mv = move[c];
        if (mv < 0 || mv > 4) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: unknown move code");
        if (mv == 0) continue;
        if (t[c] < 0 || t[c] >= e->tp.n_res || !adm.rides[t[c]])
            return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: residue type out of range or not active");
        if (!(sel_u[c] >= 0.0 && sel_u[c] < 1.0)) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: sel_u must lie in [0, 1)");
        if (mv >= 3 && !(phi_v[c] > 0.0)) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_push_gc: phi_v must be positive");
        const size_t idx = (size_t)rn.replica * e->tp.n_res + t[c];
        const int k = mv <= 2 ? MGPU_MOVE : (mv == 3 ? MGPU_CREATION : MGPU_DELETION);
        char ok = 1;
        if ((rc = admit_built(e, idx, k, mv, kAdmitFrames | kAdmitInsertion | kAdmitRange, "chain_run_push_gc", "step", c, why, ok, fast)))
            return set_error(rc, why);
    }
    for (int c = 0; c < n; ++c) {
        const size_t slot = (size_t)((rn.pushed + c) % kRunRingSteps);
        RunRec &r = rn.h_ring[slot];
        r = RunRec{};
        rn.h_gc[slot] = double2{0.0, 0.0};
        r.move = move[c];
        if (r.move == 0) continue;
        r.t = t[c]; r.m = 0; r.pad = 1;
        for (int d = 0; d < 5; ++d) r.u[d] = u5[5 * (size_t)c + d];
        r.acc_u = accept_u[c];
        rn.h_gc[slot] = double2{sel_u[c], phi_v[c]};
        // a step that is accepted may leave the fast fold's range: the flag is lowered now (mgpu_farm_window_submit's rule)
        const size_t idx = (size_t)rn.replica * e->tp.n_res + t[c];
        if (r.move != 4 && !e->frames_tight[idx]) e->in_range[idx] = 0;
    }
    rn.fast = fast;
    return run_push_copy(e, n, true);
}

int mgpu_chain_run_launch(mgpu_engine *e, int n_launches) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_launch: no run is open");
    if (n_launches < 0) return set_error(MGPU_ERR_INVALID_ARG, "chain_run_launch: negative count");
    int rc = use_device(e);
    if (rc) return rc;
    run_poll(e);
    if ((long long)(rn.seq - rn.seq_done) + n_launches > kRunMaxInFlight)
        return set_error(MGPU_ERR_STATE, "chain_run_launch: too many launches in flight (mgpu_chain_run_capacity)");
    if (e->lanes[0].n_submitted != 0) return set_error(MGPU_ERR_STATE, "chain_run_launch: lane 0 holds an un-waited trial");
    // (another path has left some replica's A(k) in its other buffer since the run was opened: back into d_A, which the run uses)
    if (e->a_switched && (rc = normalize_A(e))) return rc;
    for (int i = 0; i < n_launches; ++i)
        if ((rc = run_launch_one(e, -1, 0))) return rc;
    return MGPU_OK;
}

int mgpu_chain_run_force(mgpu_engine *e, int step, int accept) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_force: no run is open");
    if (rn.stalled_at < 0 || step != rn.stalled_at)
        return set_error(MGPU_ERR_STATE, "chain_run_force: not the step the run waits for (mgpu_chain_run_collect reports it)");
    int rc = use_device(e);
    if (rc) return rc;
    run_poll(e);
    if ((long long)(rn.seq - rn.seq_done) + 1 > kRunMaxInFlight)
        return set_error(MGPU_ERR_STATE, "chain_run_force: too many launches in flight (mgpu_chain_run_capacity)");
    if (e->a_switched && (rc = normalize_A(e))) return rc;
    // (the device writes this tag again, decided, behind the step's row)
    __atomic_store_n(&rn.h_step_tag[step % kRunRingSteps], 0ull, __ATOMIC_RELEASE);
    rn.stalled_at = -1;
    return run_launch_one(e, step, accept ? 1 : 2);
}

int mgpu_chain_run_collect(mgpu_engine *e, int max_steps, int wait, double *old_energy, double *new_energy, int *verdict, int *n_got,
                           int *stalled_at) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_collect: no run is open");
    if (max_steps < 0 || !n_got || !stalled_at || (max_steps > 0 && (!old_energy || !new_energy || !verdict)))
        return set_error(MGPU_ERR_INVALID_ARG, "chain_run_collect: bad argument");
    int rc = use_device(e);
    if (rc) return rc;
    *n_got = 0;
    *stalled_at = rn.stalled_at >= 0 ? (int)rn.stalled_at : -1;
    if (rn.stalled_at >= 0) return MGPU_OK;                   // nothing moves before mgpu_chain_run_force
    const volatile unsigned long long *tags = rn.h_step_tag;
    long long spins = 0;
    int got = 0;
    auto row = [&](long long step) {
        const double *o = rn.h_out + (size_t)(step % kRunRingSteps) * kRunOut;
        copy_energy_rows(old_energy, new_energy, got, o);
        verdict[got] = (int)o[10];
        ++got;
    };
    while (got < max_steps && rn.collected < rn.pushed) {
        const long long step = rn.collected;
        const unsigned long long decided = ((unsigned long long)(step + 1) << 1) | 1ull, tag = tags[step % kRunRingSteps];
        if (tag == decided || tag == (decided ^ 1ull)) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            row(step);
            if (tag == decided) { run_mirror(e, step); rn.collected += 1; continue; }
            rn.stalled_at = step;                                // undecided: its energies, verdict 2; the run waits for force
            *stalled_at = (int)step;
            break;
        }
        if (!wait || got > 0) break;
        __builtin_ia32_pause();
        if (++spins >= 200000 && (spins % 65536) == 0) {
            // long past any launch's run time: is anything still going to write this tag?
            const hipError_t q = hipStreamQuery(e->lanes[0].stream);
            if (q != hipSuccess && q != hipErrorNotReady) return set_error(MGPU_ERR_HIP, std::string("chain_run_collect: ") + hipGetErrorString(q));
            if (q == hipSuccess && tags[step % kRunRingSteps] == tag)
                return set_error(MGPU_ERR_STATE, "chain_run_collect: nothing in flight will produce the next step (mgpu_chain_run_launch)");
        }
    }
    *n_got = got;
    run_poll(e);
    return MGPU_OK;
}

int mgpu_chain_run_close(mgpu_engine *e) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (!rn.open) return set_error(MGPU_ERR_STATE, "chain_run_close: no run is open");
    int rc = use_device(e);
    if (rc) return rc;
    if ((rc = sync_all_lanes(e))) return rc;                    // drains lane 0; A(k) is in its primary buffer (the run never leaves it)
    run_poll(e);
    if (rn.dev_stalled) return set_error(MGPU_ERR_STATE, "chain_run_close: a step waits for the host's decision (mgpu_chain_run_force)");
    // (steps decided and never collected: the host's counts follow their insertions / deletions all the same)
    for (long long step = rn.mirrored; step < rn.pushed; ++step) {
        if (rn.h_step_tag[step % kRunRingSteps] != ((((unsigned long long)(step + 1)) << 1) | 1ull)) break;
        run_mirror(e, step);
    }
    rn.open = false;
    return MGPU_OK;
}

int mgpu_chain_run_get_stats(mgpu_engine *e, long long *launches, long long *steps, long long *void_launches, long long *undecided) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    mgpu_engine::Run &rn = e->run;
    if (rn.h_launch) run_poll(e);
    if (launches) *launches = rn.launches;
    if (steps) *steps = rn.steps;
    if (void_launches) *void_launches = rn.void_launches;
    if (undecided) *undecided = rn.undecided;
    return MGPU_OK;
}

int mgpu_chain_run_get_launches(mgpu_engine *e, int max_launches, int *first, int *consumed, int *n_got) {
    if (!e || !n_got || max_launches < 0 || (max_launches > 0 && (!first || !consumed)))
        return set_error(MGPU_ERR_INVALID_ARG, "chain_run_get_launches: bad argument");
    mgpu_engine::Run &rn = e->run;
    if (rn.h_launch) run_poll(e);
    const int n = std::min(max_launches, (int)rn.log.size());
    for (int i = 0; i < n; ++i) { first[i] = rn.log[i].first; consumed[i] = rn.log[i].second; }
    *n_got = n;
    return MGPU_OK;
}

#ifdef MGPU_FARM_STAMPS
// diagnostic builds only (tools/farm_stages.py): the last window's stamps, 3 x 8 ticks of the 100 MHz wall clock
int mgpu_farm_window_get_stamps(mgpu_engine *e, long long *out24) {
    if (!e || !out24) return set_error(MGPU_ERR_INVALID_ARG, "farm_window_get_stamps: null argument");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_farm_stamps), 24 * sizeof(long long)));
    return MGPU_OK;
}
#endif

int mgpu_farm_window_flush(mgpu_engine *e) {
    if (!e) return set_error(MGPU_ERR_INVALID_ARG, "null engine");
    int rc = use_device(e);
    if (rc) return rc;
    return sync_all_lanes(e);
}

}  // extern "C"
