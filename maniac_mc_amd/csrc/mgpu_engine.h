// Internal types of the engine's translation units: the engine object, its submission lanes, and the helpers they share.
//   mgpu_engine.hip    life cycle, replica state, structure factor, static energy, measurement
//   mgpu_launch.hip    the kernel launches (pair sweeps, reciprocal update, intra, S(k))
//   mgpu_lanes.hip     batched candidates, the asynchronous lanes (trial submit / wait / commit), the host team
//   mgpu_windows.hip   one-launch windows: a single chain (mgpu_chain_window) and a farm of chains (mgpu_farm_window_*)
#ifndef MGPU_ENGINE_H
#define MGPU_ENGINE_H

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <omp.h>
#include <string>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/maniac_gpu.h"
#include "mgpu_internal.h"
#include "mgpu_kernels.h"

namespace mgpu {

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t err__ = (expr);                                                                      \
        if (err__ != hipSuccess)                                                                        \
            return set_error(MGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));       \
    } while (0)

// grow-only device / pinned-host scratch
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need) {
        if (need <= bytes) return MGPU_OK;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr; bytes = 0;
        size_t cap = std::max<size_t>(need, 4096);
        cap += cap / 2;
        HIP_TRY(hipMalloc(&p, cap));
        bytes = cap;
        return MGPU_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
struct HostBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int reserve(size_t need) {
        if (need <= bytes) return MGPU_OK;
        if (p) HIP_TRY(hipHostFree(p));
        p = nullptr; bytes = 0;
        size_t cap = std::max<size_t>(need, 4096);
        cap += cap / 2;
        HIP_TRY(hipHostMalloc(&p, cap, hipHostMallocDefault));
        bytes = cap;
        return MGPU_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

struct ProfileSlot {
    long long launches = 0;
    double total_ms = 0.0;
};

// One submission lane: a HIP stream with its own scratch, so that work queued on one lane (for
// one group of replicas) overlaps the host's processing of the other lane's results.
// a run of items of one launch that share a reciprocal-update form (recip_groups, mgpu_launch.hip)
struct RecipGroup { int first, n, n1_max; };

struct Lane {
    hipStream_t stream = nullptr;
    DevBuf d_items, d_items2, d_sites, d_partials, d_out;
    HostBuf h_in, h_commit, h_out;   // pinned staging: trial inputs, commit inputs, results
    bool h_in_lent = false;          // h_in.p was handed to the caller (mgpu_lane_site_buffer): it must never be freed under them
    struct Pending { int kernel; hipEvent_t a, b; };
    std::vector<Pending> pending;
    struct Occupancy { const void *kernel; size_t lds; int blocks; };
    std::vector<Occupancy> occ;      // resident_blocks() cache
    // profiling state is per lane: lanes may be driven by different host threads (one thread per lane at a time)
    std::vector<hipEvent_t> ev_pool;
    ProfileSlot prof[MGPU_KERNEL_COUNT];
    int n_submitted = 0;          // candidates of the trial in flight (0 = none)
    bool dirty = false;           // something was queued on the stream since its last synchronise (asynchronous entry points)
    int last_trial_n = 0, last_trial_stride = 0;   // shape of the site rows still resident in d_sites
    bool last_trial_built = false;                 // ... built on the device (rows carry the candidates' frames)
    int last_trial_frame = 0;                      // site index of the frame inside such a row
    int n_pair_items = 0;                 // reduced pair-energy entries of the trial in flight (2 per fused item + 1 per single)
    TrialResult result{};                 // layout of its result block in d_out / h_out (mgpu_internal.h)
    // reduced pair-energy entry i sums `n_split` partials starting at double ent_off[i] of the result block, ent_stride[i]
    // doubles apart (a fused item's partials are laid out [split][state], a single item's [split])
    std::vector<int> ent_off, ent_stride, ent_ns;     // ... ent_ns[i] of them
    std::vector<char> ent_extra;          // entry i has an extra record (the framework part, pair_frozen_kernel) behind the energies
    DevBuf d_scratch;                     // chunk partials of pair_frozen_kernel
    DevBuf d_recip_sums;                  // [item][task][4]: a task's sums between the site tiles of the matrix-unit row sweep
    DevBuf d_tickets;                     // its per-group tickets: zero between launches (the kernel leaves them so)
    const RecipItem *d_trial_items = nullptr;   // RecipItems of the last trial, resident while last_trial_n != 0
    const RecipItem *h_trial_items = nullptr;   // their host image in h_in (valid until the next trial_submit)
    int trial_n1_max = 1;
    // the k sweep of the trial in flight stored every candidate's A + delta into its replica's other A(k) buffer (one
    // row-form launch, one candidate per replica), under alt_owner stamp trial_stamp: a commit of it may switch buffers
    bool trial_alt = false;
    unsigned long long trial_stamp = 0;
    // The site rows and items of the lane's previous trial are gone (overwritten, consumed by a commit, or built under rules
    // that no longer hold): nothing may be committed "from the lane's resident rows", by mask or by switching, until the next trial.
    void forget_trial() {
        last_trial_n = 0;
        d_trial_items = nullptr;
        h_trial_items = nullptr;
        trial_alt = false;
    }
    // accepted share of the lane's last commit from its resident rows: the stores pay for every candidate, the switch saves
    // the commit pass of the accepted ones only (measured alone, 4096 candidates: k sweep 38 -> 69 us, commit 40 -> 6 us)
    double accept_share = 1.0;
    // the k sweep of a trial or commit whose candidates' types take different forms (recip_groups): one launch per form,
    // the items in group order (recip_order[slot] = candidate) in their own staging blocks; recip_slot[c] = candidate c's
    // result slot in the trial in flight (empty: one group, slot = c)
    std::vector<RecipGroup> recip_groups;
    std::vector<int> recip_order, recip_slot;
    HostBuf h_recip_items;
    DevBuf d_recip_items;
    std::vector<int> pair_old, pair_new, intra_idx, kinds;   // per-candidate rows of the trial in flight
    std::vector<double> self_of;                              // per-candidate Ewald self term (host constant)
    std::vector<char> cand_ok;                                // per candidate: its sites are within the fast fold's range
    std::vector<int> build_kind;                              // candidate kinds of a device-built trial
    std::vector<double> h_lj, h_cc;                           // pair energies of the trial being collected
    std::vector<int> mark;                    // [n_replicas] scratch of the one-candidate-per-replica check
    std::vector<int> commit_mark;             // [n_replicas]: the stamp of the commit_submit_impl call that last committed there
    int commit_stamp = 0;
    // A trial whose acceptance is decided (and whose accepted candidates are committed) on the device: the flags arrive
    // with the energies; the engine's host mirrors (counts, range flags) follow when the lane is next synchronised
    int decided_n = 0;                        // candidates of such a trial not yet folded into the mirrors (0 = none)
    int decided_wait_n = 0;                   // ... whose outcomes the caller has not collected yet (mgpu_trial_decide_wait)
    hipEvent_t commit_staged_ev = nullptr;                    // recorded behind the H2D copies that read h_commit
    bool commit_staged = false;
    // Farm windows (mgpu_farm_window_submit / _wait): up to kFarmDepth windows of this lane in flight.  The host-side blocks
    // are rings (a window's records are read, and its results written, while the next window is being prepared); the
    // device scratch is shared (a stream runs its kernels one after the other).
    struct FarmWindow {
        FarmRec *h_recs = nullptr;               // pinned [kFarmDepth][cap]
        double *h_out = nullptr;                 // pinned [kFarmDepth][cap][kFarmOut]
        unsigned long long *h_tag = nullptr;     // pinned [kFarmDepth][cap]
        double2 *d_part = nullptr;               // [cap][2 nsplit]
        ChainResult *d_res = nullptr;            // [cap]
        int *d_tickets = nullptr;                // [cap], zero between launches
        int cap = 0;
        unsigned long long seq = 0;              // windows submitted so far
        struct Pending {
            unsigned long long seq;
            int n, slot;
            bool counts_change;                  // carries an insertion / deletion: must be waited before the next submit
            std::vector<int> rep, t, kind;
            std::vector<char> ok;                // the candidate's sites are within the fast fold's range
        };
        std::deque<Pending> pending;
        void release() {
            if (h_recs) (void)hipHostFree(h_recs);
            if (h_out) (void)hipHostFree(h_out);
            if (h_tag) (void)hipHostFree(h_tag);
            if (d_part) (void)hipFree(d_part);
            if (d_res) (void)hipFree(d_res);
            if (d_tickets) (void)hipFree(d_tickets);
            h_recs = nullptr; h_out = nullptr; h_tag = nullptr; d_part = nullptr; d_res = nullptr; d_tickets = nullptr;
            cap = 0;
            pending.clear();
        }
    } farm;
    void release() {
        farm.release();
        if (commit_staged_ev) { (void)hipEventDestroy(commit_staged_ev); commit_staged_ev = nullptr; }
        d_items.release(); d_items2.release(); d_sites.release(); d_partials.release(); d_out.release();
        d_scratch.release(); d_recip_sums.release();
        d_tickets.release();
        h_in.release(); h_commit.release(); h_out.release();
    }
};
constexpr int kLanes = 4;
constexpr int kFarmDepth = 4;           // farm windows a lane may have in flight
constexpr int kFarmMaxChains = 4096;   // chains per farm window
constexpr int kRunRingSteps = 4096;     // chain runs: steps pushed and not yet collected
constexpr int kRunMaxInFlight = 64;     // ... launches queued whose tags have not been read
constexpr int kRunLaunchRing = 256;     // ... their slots in pinned memory
constexpr int kRunLogMax = 1024;        // ... launches mgpu_chain_run_get_launches remembers
constexpr size_t kChainWideRowsBytes = (size_t)kChainMaxCand * kFarmWideSites * 3 * sizeof(double);   // one block of a wide window's rows

// ---- From run-time values to template instances.  A launch site picks its kernel FAMILY with ordinary ifs, states the
// family's argument list once in a generic lambda, and lets these expand the parameters that are free within the family:
// exactly the instances the calls below can name are compiled, none besides.
// with_bools(f, a, b, ...): f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...)
template <class F>
void with_bools(F &&f) { f(); }
template <class F, class... Rest>
void with_bools(F &&f, bool first, Rest... rest) {
    if (first) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
// with_int<Lo, Hi>(v, f): f(std::integral_constant<int, v>{}) for Lo <= v <= Hi; false (f not called) outside the range --
// a family's cap on a parameter is the range written at its call
template <int Lo, int Hi, class F>
bool with_int(int v, F &&f) {
    if constexpr (Lo > Hi) return false;
    else {
        if (v == Lo) { f(std::integral_constant<int, Lo>{}); return true; }
        return with_int<Lo + 1, Hi>(v, f);
    }
}
// every instance a with_bools(f, ...) over sizeof...(Free) flags can reach, for what must be done to all of them
// (hipFuncSetAttribute): the same f names them, so the two lists cannot differ
template <class F, class... Done>
void for_all_bools(F &&f, std::integral_constant<int, 0>, Done... done) { f(done...); }
template <int N, class F, class... Done>
void for_all_bools(F &&f, std::integral_constant<int, N>, Done... done) {
    for_all_bools(f, std::integral_constant<int, N - 1>{}, done..., std::false_type{});
    for_all_bools(f, std::integral_constant<int, N - 1>{}, done..., std::true_type{});
}

}  // namespace mgpu

using namespace mgpu;

struct mgpu_engine {
    int device = 0;
    int n_replicas = 0;
    Lane lanes[kLanes];
    Topo tp{};
    BoxDev bx{};
    // host copies
    std::vector<int> atoms_in_res, mol_capacity, is_active, atom_types;  // atom_types 1-based [n_res][max_atom]
    std::vector<double> charges, epsilon, sigma;
    std::vector<int> kx, ky, kz;
    std::vector<double> k2mag, form_factor, weights;
    std::vector<int> h_nmol;  // [R][n_res]
    // [R][n_res]: 1 while every site ever written for (replica, type) lies within one box length of the cell centre
    // on every axis -- the condition under which the pair sweep may fold separations with two instructions per axis
    std::vector<char> in_range;
    double rc = 0, tol = 0, alpha = 0, volume = 0;
    int box_type = 0, kmax[3] = {0, 0, 0}, nk = 0;
    double box_matrix[9]{}, bounds_lo[3]{}, reciprocal[9]{}, metrics[9]{};
    // device state
    double *d_pos = nullptr;      // [R][3][Ncap]
    int *d_nmol = nullptr;        // [R][n_res]
    double2 *d_A = nullptr;       // [R][Nk]
    int *d_kpack = nullptr;
    double *d_kw = nullptr;
    int *d_trj = nullptr;            // row form of the k list (recip_rows_kernel): packed task words,
    double2 *d_tw = nullptr;         // task weights {ff W (+j), ff W (-j)}
    int *d_kslot = nullptr;          // k (reference order) -> slot of A(k)
    std::vector<int> kslot;
    int n_slots = 0;                 // complex entries of A(k) per replica
    RecipRow *d_rrows = nullptr;
    int *d_row_first = nullptr;      // [n_rrows + 1] first task of every row (a row's tasks are contiguous): recip_rows_wide_kernel
    int n_rtasks = 0, n_rrows = 0;
    double2 *d_pair_tab = nullptr;
    char *d_coul_tab = nullptr;      // Coulomb table rows (build_coulomb_table), staged into LDS by the pair sweep
    size_t coul_bytes = 0;
    int n_cu = 256;                  // compute units of the device
    int pair_blocks_per_cu = kPairBlock >= 1024 ? 1 : 2;      // resident pair-sweep workgroups per CU (VGPR / LDS bound)
    int pair_nsplit = 1;             // waves per pair-sweep item: an engine constant (see engine_nsplit)
    std::vector<double> self_of_type; // ComputeEwaldSelfInteractionSingleMol per residue type (host constant)
    bool rows_contiguous = false;    // every row's tasks are consecutive |kz| (the matrix-unit row sweep's addressing)
    bool recip_no_mfma = false;      // MGPU_RECIP_NO_MFMA=1: many-site molecules through the vector form of the wide row sweep
    bool pair_fast_fold = true;      // two-instruction minimum-image fold where the atoms' range allows it (MGPU_PAIR_EXACT_FOLD=1: off)
    bool recip_force_per_k = false;  // MGPU_RECIP_PER_K=1: per-k reciprocal kernel even where the row form fits (tests)
    double *d_res_q = nullptr;
    int *d_res_atype = nullptr;
    // frozen residues (inactive, n1 >= 64): site_perm[t][a] = position of the caller's site a in the engine's
    // atom-type-sorted order (identity for every other residue type)
    std::vector<std::vector<int>> site_perm;
    std::vector<char> frozen;        // [n_res]
    bool any_frozen = false;
    int flat_groups = 0, flat_planes = 0;   // of the frozen layout: what pair_flat_kernel's eligibility was judged on
    int *d_atom_ty = nullptr;        // [Ncap] 0-based atom type of every slot (pair_flat_kernel fetches it per lane)
    // A frozen framework is normally the SAME in every replica (a farm copies replica 0): frozen_ref[t] = the coordinates
    // replica 0 was given (engine site order), frozen_same[r * n_res + t] = replica r holds exactly those, frozen_diff[t] =
    // replicas that do not.  Where all agree, batched trials sweep the framework with pair_frozen_kernel (candidates in the
    // lanes, the atoms scalar) -- MGPU_NO_FROZEN_BATCH=1 keeps pair_flat_kernel for it.
    std::vector<std::vector<double>> frozen_ref;
    std::vector<char> frozen_same;
    std::vector<int> frozen_diff;
    bool frozen_batch = true;
    int host_team = 1;               // host threads the per-candidate loops of submit / wait / commit may use (mgpu_set_host_team)
    // molecule frames (mgpu_replica_set_frames): com [R][3][n_mol_slots], off [R][3][Ncap]; allocated on first use
    double *d_com = nullptr, *d_off = nullptr;
    std::vector<char> frames_ok;     // [R][n_res]: the frames of (replica, type) mirror its sites
    std::vector<char> frames_tight;  // [R][n_res]: every molecule's centre lies in the cell and its offsets within 0.24 L:
                                     // any device-built candidate then lies within the fast fold's range
    std::vector<char> frames_held;   // [R][n_res]: slot 0's frame holds a molecule's offsets (set_frames gave one; a deletion
                                     // leaves them): a device-built insertion copies them whatever the count
                                     // (create_molecule.f90:196-200), and is refused where this is 0
    // reservoirs (mgpu_replica_set_reservoir), allocated on first use: rsv_ptr[r * n_res + t] = the device block
    // [rsv_cap][n1][3] (null: none) whose table d_rsv the kernels read (Topo::rsv), d_rsv_nc = {count, capacity} per entry
    // (the count lives on the device only: the device-built paths change it); rsv_tight = every offset the reservoir was
    // given lies within frames_tight's bound (frames_tight of the type includes it)
    std::vector<double *> rsv_ptr;
    std::vector<int> rsv_cap;
    std::vector<char> rsv_tight;
    double **d_rsv = nullptr;
    int *d_rsv_nc = nullptr;
    bool tri_moves = false;          // mgpu_set_triclinic_moves: a triclinic engine builds moves on the device and takes farm windows
    bool wide_tri = false;           // mgpu_chain_set_wide_triclinic: the single-chain one-launch paths take types of 6..63 sites in this triclinic box
    bool farm_wide_tri = false;      // mgpu_farm_set_wide_triclinic: farm windows take types of 6..63 sites in this triclinic box
    bool rsv_any = false;            // some reservoir was set: device-built rows carry the pick (reservoir_row_pick)
    // Register-site sweeps of this engine go through pair_flat_kernel (one software-pipelined loop over all units of
    // a work unit) instead of the plane-by-plane pair_sweep_kernel: chosen at creation for topologies with short planes
    // (every plane-major residue type has at most kFlatMaxCap molecule slots) or a frozen residue; MGPU_PAIR_FLAT=0 / 1
    // overrides (tuning / A-B).  Orthorhombic boxes only; a site-major ACTIVE residue (n1 >= 64) keeps the other kernel.
    bool pair_flat = false;
    int *d_atom_res = nullptr, *d_atom_mol = nullptr;
    double *d_atom_q = nullptr;
    double *d_atom_q_on = nullptr;   // the same with charges below CoulombEnergy's threshold set to zero (pair_frozen_kernel's scalars)
    double2 *d_phase_tab = nullptr;  // [ktot][Ncap] scratch for S(k)
    double2 *d_S = nullptr;          // [Nk] scratch
    // lane 0 doubles as the synchronous path's stream and scratch
    hipStream_t &stream = lanes[0].stream;
    DevBuf &d_items = lanes[0].d_items, &d_items2 = lanes[0].d_items2, &d_sites = lanes[0].d_sites,
           &d_partials = lanes[0].d_partials, &d_out = lanes[0].d_out;
    HostBuf &h_out = lanes[0].h_out;
    HostBuf h_stage;
    // farm snapshots (mgpu_farm_snapshot_submit / _wait): the item table, the gathered block on the device and its pinned
    // host copy, which the caller reads after the wait
    DevBuf d_snap, d_snap_items;
    HostBuf h_snap, h_snap_items;
    size_t snap_bytes = 0;
    bool snap_pending = false;
    // state blocks (mgpu_state_export_submit / _wait, mgpu_state_import): the item table, the block on the device and the
    // pinned host copy of an export, which the caller reads after the wait
    DevBuf d_state, d_state_items;
    HostBuf h_state, h_state_items;
    size_t state_bytes = 0;
    bool state_pending = false;
    // single-chain windows (mgpu_chain_window): pinned, host-coherent blocks the kernel reads its candidates from and
    // writes its results to (no copies, no stream synchronisation: the host polls the tag), and device scratch
    struct Chain {
        double *h_out = nullptr;                     // [kChainMaxCand][10] energies | first, undecided | stage stamps
        unsigned long long *h_tag = nullptr;
        Topo *d_topo = nullptr;                      // the engine's Topo in device memory (the kernel indexes it by loaded residue types)
        bool topo_stale = true;
        ChainResult *d_res = nullptr;
        double2 *d_part = nullptr;
        double2 *d_alt = nullptr;                    // [kChainMaxCand][n_slots]: A + delta of every candidate of the window
        int *d_ticket = nullptr;
        unsigned long long seq = 0;
        double margin = 16.0 * 2.220446049250313e-16;   // relative band around the acceptance probability left to the host's exp
        long long windows = 0, undecided = 0;
        bool timing = false;                         // stage stamps wanted (mgpu_chain_set_timing)
        bool wide = false;                           // windows take rows of 6..63 sites (mgpu_chain_set_wide)
        double *h_rows = nullptr;                    // pinned [2][kChainMaxCand][kFarmWideSites][3]: such rows, the blocks taken in turn
    } chain;
    // The A(k) double buffer: the other buffer of every replica and which of the two is its current one (d_acur[r] = 1:
    // d_A_alt), allocated on first use (alt_reserve).  Farm windows and the batched trials store every candidate's A + delta into
    // the other buffer, and an accepted candidate is committed by making that buffer current.  `a_switched` = some replica's
    // current A(k) may live in d_A_alt: the synchronous entry points copy it back into d_A first (normalize_A); the kernels of
    // the lanes pick each replica's current buffer themselves (RecipA).
    double2 *d_A_alt = nullptr;
    int *d_acur = nullptr;
    std::atomic<bool> a_switched{false};
    // alt_owner[r]: the stamp of the batched trial whose A + delta replica r's other buffer holds (0: none -- anything else
    // that rewrote the replica's state since clears it); trial_stamps hands the stamps out.  Entries are written by the lanes'
    // driver threads (each for its own replicas): relaxed atomic accesses.
    std::vector<unsigned long long> alt_owner;
    std::atomic<unsigned long long> trial_stamps{0};
    bool commit_pass = false;        // MGPU_COMMIT_PASS=1: every commit recomputes A + delta (no commit by switching; tests, A/B)
    std::mutex alt_mu;               // the double buffer's first allocation
    // farm windows (mgpu_farm_window_*): the per-replica stall flag, allocated on first use, and the window counters
    struct Farm {
        int *d_stalled = nullptr;
        std::atomic<long long> windows{0}, undecided{0};   // (the lanes may be driven by different host threads)
        std::mutex mu;                                     // the engine-wide blocks' first allocation
    } farm;
    // What the one-launch paths make of every residue type (window_types_build, mgpu_windows.hip): built when the engine is
    // created, from values fixed there (n1, site_major, the box, kmax, the row structure, MGPU_RECIP_NO_MFMA / _PER_K).
    struct WindowTypes {
        signed char take[kMaxRes];                   // kWindowNone / kWindowNarrow (<= kMaxFusedSitesWide sites, row form) / kWindowWide
        signed char kform[kMaxRes];                  // the k role's form (kFarmForm*), its rows per tile and site-states
        int wide_rpt[kMaxRes], wide_nss[kMaxRes];
        size_t k_lds[kMaxRes];                       // the k role's dynamic LDS (window_k_lds_bytes)
        size_t k_lds_one, k_lds_max;                 // ... of a one-site row (the floor of a narrow launch), over the types a row may carry
        // a triclinic box: what a type of 6..63 sites would take with the image-search WIDE instances (chain_window_kernel<false,
        // false, true, true>, chain_run_kernel<false, false, true, GC, true>) -- kWindowWide or kWindowNone, by the orthorhombic
        // rule; kform, wide_rpt, wide_nss and k_lds of such a type are recorded either way.  Read by kPathChain and kPathRun
        // under mgpu_chain_set_wide_triclinic and by kPathFarm (farm_window_kernel<false, false, true, RSV, true>) under
        // mgpu_farm_set_wide_triclinic; k_lds_max_tri = k_lds_max with these types counted.
        signed char take_tri[kMaxRes];
        size_t k_lds_max_tri;
        bool rows_one;                               // a one-site molecule takes the row form (single-chain windows without a narrow active type)
    } win{};
    // a chain run (mgpu_chain_run_*): launches of one chain queued back to back on lane 0, each continuing from the cursor in
    // device memory (chain_run_kernel).  Single-driver: one host thread opens, pushes, launches, collects and closes a run.
    struct Run {
        bool open = false;
        bool triclinic = false;                      // a triclinic box takes runs (mgpu_chain_run_set_triclinic; needs tri_moves)
        bool wide = false;                           // runs take types of 6..63 sites (mgpu_chain_run_set_wide: the WIDE instances)
        int replica = -1, k = 0;
        double t_step = 0.0, r_step = 0.0, temperature = 0.0;
        bool fast = false;                           // every record so far admits the fast fold
        RunState *d_state = nullptr;
        RunRec *d_ring = nullptr, *h_ring = nullptr; // device ring and its pinned image (the source of the pushes' copies)
        bool gc = false;                             // grand-canonical runs (mgpu_chain_run_set_gc): by-count records, the GC instances
        double2 *d_gc = nullptr, *h_gc = nullptr;    // ... their second ring {sel_u, phi V} and its pinned image (allocated with the first such run)
        long long mirrored = 0;                      // steps whose accepted insertions / deletions the host's counts have followed
        int *h_pushed = nullptr;                     // pinned [kRunRingSteps]: the counts the pushes copy into d_state->pushed
        double *h_out = nullptr;                     // pinned [kRunRingSteps][kRunOut]
        unsigned long long *h_step_tag = nullptr;    // pinned [kRunRingSteps]
        unsigned long long *h_launch = nullptr;      // pinned [2][kRunLaunchRing]: info | tag
        double2 *d_part = nullptr, *d_alt = nullptr;
        ChainResult *d_res = nullptr;
        int *d_ticket = nullptr;
        long long pushed = 0, collected = 0;         // steps
        long long stalled_at = -1;                   // the undecided step collect has reported and force has not yet answered
        bool dev_stalled = false;                    // the stall flag as the last launch seen left it
        unsigned long long seq = 0, seq_done = 0;    // launches queued / whose tags have been read (never reset)
        long long launches = 0, steps = 0, void_launches = 0, undecided = 0;
        std::deque<std::pair<int, int>> log;         // (first, consumed) of the last launches seen since open
    } run;
    // radial distribution functions (mgpu_rdf_*, mgpu_replicas.hip): the selection, and the accumulators of every replica --
    // d_acc = hist [R][n_pairs][n_bins] | eligible [R][n_pairs] | samples [R], unsigned long long, as `acc` describes it
    // (mgpu_internal.h); d_tab = the RdfTable.  Nothing but the mgpu_rdf_* calls touches them.
    struct Rdf {
        int n_bins = 0, n_pairs = 0, include_intra = 0;       // n_pairs = 0: not configured
        double r_max = 0.0, r_max2 = 0.0, inv_dr = 0.0;
        int type_a[8]{}, type_b[8]{};
        Accum acc;
        DevBuf d_acc, d_tab;
    } rdf;
    // density maps (mgpu_density_*, mgpu_replicas.hip): the grid, the channels' atom types, every replica's group, and the
    // accumulators -- d_acc = hist [n_groups][n_channels][n2][n1][n0] | samples [n_groups], unsigned long long, as `acc`
    // describes it; d_group = group_of [R].  Nothing but the mgpu_density_* calls touches them.
    struct Density {
        int n[3]{}, n_channels = 0, n_groups = 0;             // n_channels = 0: not configured
        int types[8]{};
        unsigned long long table = ~0ull;                     // atom type -> channel, a nibble each (0xF: none)
        Accum acc;
        DevBuf d_acc, d_group;
    } density;
    // per-molecule removal energies (mgpu_molecule_energy_*, mgpu_replicas.hip): the bins, the selected residue types, and the
    // accumulators of every replica -- d_acc = hist [R][n_sel][n_bins + 2] | samples [R], unsigned long long, as `acc`
    // describes it.  Nothing but the mgpu_molecule_energy_* calls touches them.
    struct MolEnergy {
        int n_bins = 0, n_sel = 0;                            // n_sel = 0: not configured
        double e_min = 0.0, e_max = 0.0, inv_w = 0.0;
        int types[8]{};
        Accum acc;
        DevBuf d_acc;
    } molen;
    // profiling
    bool profiling = false;
};

namespace mgpu {

const char *last_error_text();
int use_device(const mgpu_engine *e);
int prof_begin(mgpu_engine *e, Lane &ln, int kernel, hipEvent_t *a, hipEvent_t *b);
int prof_end(mgpu_engine *e, Lane &ln, int kernel, hipEvent_t a, hipEvent_t b);
int prof_collect(mgpu_engine *e, Lane &ln);
void finish_decided(mgpu_engine *e, Lane &ln);
void frozen_changed(mgpu_engine *e, int replica, int t);
int sync_lane(mgpu_engine *e, Lane &ln);
int sync_stream(mgpu_engine *e);
int sync_all_lanes(mgpu_engine *e);
int check_candidate(const mgpu_engine *e, int c, int replica, int t, int m, bool need_resident);
bool sites_in_range(const mgpu_engine *e, const double *sites, int n_sites);
bool replica_in_range(const mgpu_engine *e, int replica);
// (replica, t) has a reservoir (mgpu_replica_set_reservoir): its insertions copy reservoir molecules, not slot 0's frame
inline bool has_reservoir(const mgpu_engine *e, size_t idx) { return !e->rsv_ptr.empty() && e->rsv_ptr[idx] != nullptr; }
// Admission of device-built candidate c (kind k, move code mv; idx = replica * n_res + type) to a batched trial or a farm window:
// MGPU_OK, or the refusal's code with its text ("<who>: ... <noun> c") in `msg`.  `checks` picks the refusals to test, in this
// order -- a farm window tests its molecule pick between the frames and the insertion, so it asks twice.  kAdmitRange: a built
// candidate's centre lies in the cell (ApplyPBC / uniform insertion), so with tight frames its sites are within the fast fold's
// range -- `ok` reports that, and `fast` is lowered with it.
enum { kAdmitFrames = 1, kAdmitMove = 2, kAdmitInsertion = 4, kAdmitRange = 8, kAdmitAll = 15 };
inline int admit_built(const mgpu_engine *e, size_t idx, int k, int mv, int checks, const char *who, const char *noun, int c,
                       std::string &msg, char &ok, bool &fast) {
    if ((checks & kAdmitFrames) && (!e->d_com || !e->frames_ok[idx])) {
        msg = std::string(who) + ": no molecule frames for " + noun + " " + std::to_string(c) + " (mgpu_replica_set_frames)";
        return MGPU_ERR_STATE;
    }
    if ((checks & kAdmitMove) && (mv < 1 || mv > 4 || (k == MGPU_MOVE) != (mv <= 2) || (k == MGPU_CREATION) != (mv == 3))) {
        msg = std::string(who) + ": move code does not match the candidate kind";
        return MGPU_ERR_INVALID_ARG;
    }
    // the insertion copies slot 0's frame whatever the count (create_molecule.f90:196-200), which a deletion leaves in place:
    // there must be one (a type with a reservoir copies a reservoir molecule instead)
    if ((checks & kAdmitInsertion) && k == MGPU_CREATION && !e->frames_held[idx] && !has_reservoir(e, idx)) {
        msg = std::string(who) + ": an insertion copies the geometry of molecule 1 of its type, and this type has never held one on this replica";
        return MGPU_ERR_STATE;
    }
    if ((checks & kAdmitRange) && k != MGPU_DELETION) { ok = e->frames_tight[idx]; fast = fast && ok; }
    return MGPU_OK;
}
int engine_nsplit(const mgpu_engine *e);
void permute_frozen_rows(const mgpu_engine *e, double *rows, int n_rows, int site_stride, const int *t);
bool any_frozen(const mgpu_engine *e, int n, const int *t);
int upload_sites(Lane &ln, const double *sites, int n_rows, int site_stride);
int upload_sites(mgpu_engine *e, const double *sites, int n_rows, int site_stride, const int *t);
double self_energy_host(const mgpu_engine *e, int t);
int normalize_A(mgpu_engine *e);                // every replica's current A(k) back into d_A (mgpu_windows.hip)
int alt_reserve(mgpu_engine *e);                // the A(k) double buffer (mgpu_windows.hip)
void alt_forget(mgpu_engine *e, int replica);   // replica's other buffer holds nothing a commit may switch to (-1: every replica)
// at most one of the n records per replica?  false: some replica (all within [0, n_replicas)) occurs twice
bool one_record_per_replica(Lane &ln, int n_replicas, const int *replica, int n);
// spin until each of the n pinned tags shows seq (then the results behind them are visible); from `first_check` spins on,
// every `check_every`, make sure the stream is still alive.  `what` heads the error text.
int wait_for_tag(hipStream_t stream, const volatile unsigned long long *tag, int n, unsigned long long seq, long long first_check,
                 long long check_every, const char *what);
int farm_clear_stall(mgpu_engine *e, int replica);   // the replica's state was rewritten: it waits for no decision (mgpu_windows.hip)
int chain_topo(mgpu_engine *e, const Topo **d_topo);   // the engine's Topo in device memory (mgpu_windows.hip)
void chain_run_release(mgpu_engine *e);                // a chain run's blocks (mgpu_windows.hip)
enum { kWindowNone = 0, kWindowNarrow = 1, kWindowWide = 2 };
void window_types_build(mgpu_engine *e);               // e->win, at the end of mgpu_engine_create (mgpu_windows.hip)
// mgpu_launch.hip
int launch_pair(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, int common_n1, int site_stride,
                int nsplit, double *d_lj, double *d_c, bool ordered = false, double2 *host_partials = nullptr,
                bool fused = false, bool fast_fold = false, bool skip_frozen = false);
int frozen_chunk_atoms(const mgpu_engine *e, int n_atoms);
int launch_frozen(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, int n1, int site_stride, bool fused, bool fast_fold,
                  int t_frozen, double2 *d_scratch, double2 *d_extra);
// the lane blocks of a batched trial with the engine's record sizes (the arithmetic: mgpu_internal.h)
static_assert((3 * sizeof(PairItem) + sizeof(RecipItem)) % 8 == 0, "the items end 8-byte aligned: TrialStaging::moves is their end");
inline TrialStaging trial_staging(int n, int site_stride, bool built, bool reservoir_pick, bool decide) {
    return trial_staging<sizeof(PairItem), sizeof(RecipItem), sizeof(DecideItem)>(n, site_stride, built, reservoir_pick, decide);
}
inline size_t lane_site_buffer_bytes(int n_max, int site_stride) {
    return lane_site_buffer_bytes<sizeof(PairItem), sizeof(RecipItem), sizeof(DecideItem)>(n_max, site_stride);
}
// the engine's dynamic-LDS sizes (the arithmetic: mgpu_internal.h)
static_assert(sizeof(double2) == kLdsPhase && sizeof(int4) == kLdsRowRec, "mgpu_internal.h sizes the LDS tables with these");
inline int recip_ktot(const mgpu_engine *e) { return recip_ktot(e->kmax); }
inline size_t recip_rows_lds_bytes(const mgpu_engine *e, int n1_max) { return recip_rows_lds_bytes(recip_ktot(e), e->n_rrows, n1_max); }
static_assert(kWindowPairWaves == kPairWaves && kWindowSiteChunk == kSiteChunk, "mgpu_internal.h sizes the windows' LDS with these");
bool recip_by_rows(const mgpu_engine *e, int n1_max);
struct RecipPlan {
    int form = MGPU_RECIP_FORM_ROWS;   // MGPU_RECIP_FORM_*
    bool by_rows = true;
    int tile = 1;                      // row form: n1_max; per-k form: sites per LDS tile
    int mfma_tile = 0;                 // matrix-unit wide form: site-states per LDS tile (else 0)
    int wide_rpt = 0;                  // vector wide form: rows per XY tile (else 0)
    int wide_nss = 0;                  // either wide form: site-states in LDS at a time (else 0)
    size_t lds = 0;                    // dynamic LDS of the row / per-k kernel: beyond kLdsDefaultMax kmax is too large for the engine
    size_t wide_lds = 0;               // dynamic LDS of the wide kernel (either wide form)
};
RecipPlan recip_plan(const mgpu_engine *e, int n1_max, bool wide_ok);
void recip_groups(const mgpu_engine *e, const RecipItem *items, int n, std::vector<RecipGroup> &groups, std::vector<int> &order);
int launch_recip(mgpu_engine *e, Lane &ln, const RecipItem *d_items, int n_items, int n1_max, int site_stride,
                 bool commit, double2 *A_base, double *d_u, double *d_u_old = nullptr, const AcceptBits *accept = nullptr,
                 const double *sites_override = nullptr, const DecideArgs *decide = nullptr, bool store_alt = false);
int launch_commit_switch(mgpu_engine *e, Lane &ln, const RecipItem *d_items, int n_items, int site_stride, const AcceptBits &accept);
int launch_sfactor(mgpu_engine *e, int replica, double2 *dst);
int launch_intra(mgpu_engine *e, Lane &ln, const PairItem *d_items, int n_items, const double *d_sites, int site_stride, double *d_out);

// The per-candidate loops of a submit / wait / commit are cut into `parts` contiguous ranges (boundaries on multiples of
// 32 candidates: the commit's accept mask is built a word per range) and run by an OpenMP team of the calling thread --
// the same runtime as the Fortran drivers', whose nested hot team is reused.  One part = the serial loop.
constexpr int kHostPartMin = 1024;          // candidates below which a team is not worth waking
constexpr int kMaxHostParts = 16;
static int host_parts(const mgpu_engine *e, int n) {
    return (e->host_team > 1 && n >= kHostPartMin) ? std::min(e->host_team, kMaxHostParts) : 1;
}
static void part_range(int n, int parts, int part, int &c0, int &c1) {
    const int words = (n + 31) / 32;
    c0 = std::min(n, (int)((long long)words * part / parts) * 32);
    c1 = std::min(n, (int)((long long)words * (part + 1) / parts) * 32);
}
template <class F>
static void for_parts(int parts, F &&f) {
    if (parts <= 1) { f(0); return; }
#pragma omp parallel for num_threads(parts) schedule(static, 1)
    for (int part = 0; part < parts; ++part) f(part);
}
// what a part has to say when a candidate is refused: the caller reports the lowest candidate's message (the serial loop's)
struct PartError {
    int c = -1, rc = MGPU_OK;
    std::string msg;
    void set(int cand, int code, const std::string &m) { if (c < 0) { c = cand; rc = code; msg = m; } }
};
static int report_first(const PartError *errs, int parts) {
    const PartError *first = nullptr;
    for (int q = 0; q < parts; ++q)
        if (errs[q].c >= 0 && (!first || errs[q].c < first->c)) first = &errs[q];
    return first ? set_error(first->rc, first->msg) : MGPU_OK;
}

// sites per item if all items agree, else 0
template <class Item>
int common_site_count(const mgpu_engine *e, const std::vector<Item> &items) {
    int n1 = 0;
    for (const auto &it : items) {
        const int v = e->tp.n1[it.t];
        if (n1 == 0) n1 = v;
        else if (n1 != v) return 0;
    }
    return n1;
}

}  // namespace mgpu

#endif
