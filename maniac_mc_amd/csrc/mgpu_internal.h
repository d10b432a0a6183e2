// Internal declarations shared by the host-setup and engine translation units.
#ifndef MGPU_INTERNAL_H
#define MGPU_INTERNAL_H

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace mgpu {

// /root/reference/src/constants.f90:7-20 -- same decimal literals, so bit-identical doubles
constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;
constexpr double kEps0InvEvA = 14.40198;
constexpr double kKbEvK = 8.6173852e-5;
constexpr double kErrorTol = 1.0e-10;

// records `msg` as the calling thread's last error and returns `code`
int set_error(int code, const std::string &msg);

int box_prepare(const double m[9], int *box_type, double *volume, double rcp[9], double metrics[9]);
int ewald_setup(const double metrics[9], double *rc, double *tol, double *alpha, double *screening,
                double *fourier_precision, int kmax[3], int *nk);
int ewald_kvectors(const double rcp[9], double alpha, const int kmax[3], int nk, int *kx, int *ky, int *kz,
                   double *k2mag, double *ff, double *w);

// Coulomb table rows (see build_coulomb_table in mgpu_host_setup.cpp): the row index is the binary exponent and the top
// kCoulM = 6 mantissa bits of r^2 (64 rows per octave); a row is a degree-6 polynomial, 5 fp64 + 2 fp32 coefficients =
// three 16-byte LDS reads.  (128 rows per octave with degree-5 rows and 256 with 32-byte degree-4 rows were built and
// measured in rounds 2-3: 2-3 % at twice / four times the LDS; LABNOTES.md.)
constexpr int kCoulM = 6;
constexpr int kCoulDeg = 6;                        // polynomial degree of a row
constexpr int kCoulEmin = -2;                      // table starts at r^2 = 2^kCoulEmin (r = 0.5 A); below it the slow path runs
constexpr double kCoulSlowBelow = 0.25;
struct CoulRow {
    double c[5];
    float c5, c6;
};
static_assert(sizeof(CoulRow) == 48, "CoulRow must be three 16-byte LDS reads");
constexpr int kCoulRowVec = sizeof(CoulRow) / 16;  // 16-byte LDS reads per row
// the shared far row starts where kCoulKelvin * G(s) <= kCoulFarKelvin: a tenth of the 1e-11 K per unit charge product the
// table is held to beyond alpha r = 1 (tests/test_coulomb_table.py)
constexpr double kCoulKelvin = 167101.0;           // K A per unit charge product (the bound's scale, not the engine's constant)
constexpr double kCoulFarKelvin = 1.0e-12;
int build_coulomb_table(double alpha, double s_max, std::vector<CoulRow> &rows, int *idx_base, int *box_last_row = nullptr);
double coulomb_table_eval_host(const std::vector<CoulRow> &rows, int idx_base, double alpha, double s);

// ---- Dynamic LDS of the reciprocal kernels: the one home of this arithmetic (plain integers: the host tests compile it
// without a device).  The layouts these sizes describe are the kernels' (mgpu_kernels_recip.h); a size that disagrees with
// them is an out-of-bounds LDS access, so nothing outside this block recomputes one.
constexpr size_t kLdsDefaultMax = 64 * 1024;       // dynamic LDS a kernel gets without opting in to more
constexpr size_t kLdsPhase = 16, kLdsRowRec = 16;  // a phase-table entry (double2), a row record of the matrix-unit form (int4)
inline int recip_ktot(const int kmax[3]) { return kmax[0] + kmax[1] + kmax[2] + 3; }      // 1-D phases per site and state
// recip_kernel / recip_rows_kernel: the 1-D phase tables of both states of n1 sites and the sites' charges ...
inline size_t recip_lds_bytes(int ktot, int n1) { return (size_t)2 * n1 * ktot * kLdsPhase + (size_t)n1 * sizeof(double); }
// ... and, row form, the XY table: every row of every site-state
inline size_t recip_rows_lds_bytes(int ktot, int n_rrows, int n1) {
    return recip_lds_bytes(ktot, n1) + (size_t)n_rrows * (2 * n1 * kLdsPhase);
}
// recip_rows_wide_kernel (and the WIDE farm windows' k role behind kFarmKFront): the 1-D tables and charges of `nss`
// site-states, the XY table of `rpt` rows of them (vector form) or the row records (matrix-unit form)
inline size_t recip_wide_lds_bytes(int ktot, int n_rrows, size_t nss, int rpt, bool mfma) {
    return nss * ktot * kLdsPhase + (size_t)rpt * nss * kLdsPhase + nss * sizeof(double) + (mfma ? (size_t)n_rrows * kLdsRowRec : 0);
}
constexpr size_t kRecipTileBytes = 48 * 1024;       // per-k form: both table sets of a tile of sites
constexpr size_t kRecipRowsLdsMax = 40 * 1024;      // row form: while everything fits this
constexpr size_t kRecipWideTableBytes = 40 * 1024, kRecipWideLdsBytes = 60 * 1024;   // (dynamic LDS: 64 KiB with the static part)
// sites per LDS tile of the per-k form: as many as fit kRecipTileBytes, at least one
inline int recip_tile_sites(int ktot, int n1_max) {
    return std::max(1, std::min(n1_max, (int)(kRecipTileBytes / recip_lds_bytes(ktot, 1))));
}
// vector wide form: rows per XY tile (0: tables beyond kRecipWideTableBytes, or fewer than eight rows per tile)
inline int recip_wide_rows_per_tile(int ktot, int n_rrows, int n1_max) {
    const size_t nss = (size_t)2 * n1_max, tables = recip_wide_lds_bytes(ktot, 0, nss, 0, false);
    if (tables > kRecipWideTableBytes) return 0;
    const int rpt = (int)((kRecipWideLdsBytes - tables) / (nss * kLdsPhase));
    return rpt >= 8 ? std::min(rpt, n_rrows) : 0;
}
// matrix-unit wide form: site-states per tile, a multiple of four (0: not even four fit) -- the fewest tiles of at most
// kRecipWideLdsBytes each, balanced
inline int recip_wide_mfma_tile(int ktot, int n_rrows, int n1_max) {
    const size_t nss = ((size_t)2 * n1_max + 3) & ~(size_t)3;
    const size_t per_ss = recip_wide_lds_bytes(ktot, 0, 1, 0, false), fixed = recip_wide_lds_bytes(ktot, n_rrows, 0, 0, true);
    if (fixed + 4 * per_ss > kRecipWideLdsBytes) return 0;
    const size_t fit = ((kRecipWideLdsBytes - fixed) / per_ss) & ~(size_t)3;
    const size_t n_tiles = (nss + fit - 1) / fit;
    return (int)((((nss + n_tiles - 1) / n_tiles) + 3) & ~(size_t)3);
}

// ---- Dynamic LDS of a WIDE single-chain window (chain_window_kernel<..., WIDE>, mgpu_kernels_windows.h): a launch gets the
// largest of its roles' needs.  A row of a type of more than five sites is staged in LDS with a stride of kWideRowSites sites.
constexpr int kWideRowSites = 64;
// k role of such a row: candidate row | the intra wave's two tiles of {x, y, z, q} | the tables of the type's form
constexpr size_t wide_k_front_bytes() { return (size_t)kWideRowSites * 3 * sizeof(double) + 2 * (size_t)kWideRowSites * 4 * sizeof(double); }
inline size_t chain_wide_k_lds_bytes(size_t form_bytes) { return wide_k_front_bytes() + form_bytes; }
// pair role: the Coulomb table (rounded up to 16 bytes: chain_wide_pair_at), then per wave a candidate row, a slab of
// site_chunk sites {x, y, z, q} and their atom types (the NS = 0 sweep's)
inline size_t chain_wide_pair_at(size_t coul_bytes) { return (coul_bytes + 15) & ~(size_t)15; }
constexpr size_t wide_pair_slab_bytes(int pair_waves, int site_chunk) {
    return (size_t)pair_waves * (((size_t)kWideRowSites * 3 + (size_t)site_chunk * 4) * sizeof(double) + (size_t)site_chunk * sizeof(int));
}
inline size_t chain_wide_pair_lds_bytes(size_t coul_bytes, int pair_waves, int site_chunk) {
    return chain_wide_pair_at(coul_bytes) + wide_pair_slab_bytes(pair_waves, site_chunk);
}
// resolving workgroup (every instance): the split partials {lj, coulomb} of the window's pair entries
inline size_t chain_resolver_lds_bytes(int n_ent, int nsplit) { return (size_t)n_ent * nsplit * kLdsPhase; }
// largest window the resolver's staging admits within the default budget: two entries per step
inline int chain_window_steps_by_lds(int nsplit) { return (int)(kLdsDefaultMax / chain_resolver_lds_bytes(2, nsplit)); }
// a chain-run launch of k steps (chain_run_kernel): its resolver stages both entries of every step
inline size_t chain_run_resolver_lds_bytes(int k, int nsplit) { return chain_resolver_lds_bytes(2 * k, nsplit); }

// ---- Dynamic LDS of a launch of the three one-launch paths (mgpu_windows.hip), narrow and WIDE: the largest of its roles'
// needs.  The launch sites and the capacity rules take every size and both budget comparisons from here.
enum WindowPath { kPathChain, kPathFarm, kPathRun };   // mgpu_chain_window, mgpu_farm_window_*, mgpu_chain_run_*
constexpr int kWindowPairWaves = 8, kWindowSiteChunk = 32;   // kPairWaves, kSiteChunk (asserted in mgpu_engine.h)
// gfx950 gives a workgroup up to 160 KiB; the WIDE instances, which opt in beyond 64 KiB, leave kFarmWideStaticMax to their static LDS
constexpr size_t kFarmWideStaticMax = 16 * 1024, kFarmWideLdsMax = 160 * 1024 - kFarmWideStaticMax;
inline size_t window_lds_budget(bool wide) { return wide ? kFarmWideLdsMax : kLdsDefaultMax; }
// pair role: the Coulomb table, and behind it (WIDE) the waves' rows and slabs
inline size_t window_pair_lds_bytes(bool wide, size_t coul_bytes) {
    return wide ? chain_wide_pair_lds_bytes(coul_bytes, kWindowPairWaves, kWindowSiteChunk) : coul_bytes;
}
// k role of a row by its type's form: the row form's tables (recip_rows_lds_bytes) for a narrow row, the front and the form's
// tables (row form, or recip_wide_lds_bytes) for a row of more than five sites
inline size_t window_k_lds_bytes(bool wide_row, size_t form_bytes) { return wide_row ? chain_wide_k_lds_bytes(form_bytes) : form_bytes; }
// the resolving waves' scratch of a farm window: four sums per split and four more, per wave
inline size_t farm_resolver_scratch_bytes(int nsplit) { return (size_t)kWindowPairWaves * (4 * nsplit + 4) * sizeof(double); }
// resolver: `count` = pair entries of a single-chain window, steps of a chain-run launch; a farm's does not depend on its chains
inline size_t window_resolver_lds_bytes(WindowPath path, int count, int nsplit) {
    return path == kPathChain ? chain_resolver_lds_bytes(count, nsplit)
                              : (path == kPathFarm ? farm_resolver_scratch_bytes(nsplit) : chain_run_resolver_lds_bytes(count, nsplit));
}
// the launch: k_bytes = the largest k role (window_k_lds_bytes) among the rows it carries -- narrow -- or may carry -- WIDE
inline size_t window_lds_bytes(WindowPath path, bool wide, size_t coul_bytes, size_t k_bytes, int count, int nsplit) {
    return std::max(std::max(window_pair_lds_bytes(wide, coul_bytes), k_bytes), window_resolver_lds_bytes(path, count, nsplit));
}
inline bool window_lds_fits(bool wide, size_t lds) { return lds <= window_lds_budget(wide); }

// ---- The two blocks of a batched trial on a lane (mgpu_lanes.hip): the one home of their layouts, plain integers as above.
// trial_submit_impl, trial_wait_impl, finish_decided and the DecideItem offsets take every offset from here: a block that
// disagrees between writer and reader gives a wrong energy, not a crash (tests/test_trial_layout.py).
// The pinned staging block, copied to the device as it stands (byte offsets; PairB, RecipB, DecideB = sizeof PairItem, RecipItem,
// DecideItem): [site rows | 2n pair items | n k items | n intra items | move codes (n ints) | 5n uniforms | n decide items].
// Host rows have `site_stride` sites; a row built on the device is [sites | com | offsets (| reservoir pick)] of the largest
// molecule (`site_stride` sites).  Move codes and uniforms: device-built trials only; decide items: the deciding form only;
// both start 8-byte aligned.
struct TrialStaging {
    int row_sites, frame_at, pick_at;   // sites per row; built rows: site index of the frame (com) and of the reservoir pick (0: none)
    size_t sites, pair_items, k_items, intra_items, moves, uniforms, decide_items, total;
};
template <size_t PairB, size_t RecipB, size_t DecideB>
inline TrialStaging trial_staging(int n, int site_stride, bool built, bool reservoir_pick, bool decide) {
    const auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    TrialStaging s{};
    s.row_sites = built ? 2 * site_stride + 1 + (reservoir_pick ? 1 : 0) : site_stride;
    s.frame_at = built ? site_stride : 0;
    s.pick_at = built && reservoir_pick ? 2 * site_stride + 1 : 0;
    s.pair_items = (size_t)n * s.row_sites * 3 * sizeof(double);
    s.k_items = s.pair_items + 2 * (size_t)n * PairB;
    s.intra_items = s.k_items + (size_t)n * RecipB;
    s.moves = up8(s.intra_items + (size_t)n * PairB);
    s.uniforms = s.moves + up8((size_t)n * sizeof(int));
    s.decide_items = up8(built ? s.uniforms + (size_t)5 * n * sizeof(double) : s.moves);
    s.total = s.decide_items + (decide ? (size_t)n * DecideB : 0);
    return s;
}
// What mgpu_lane_site_buffer reserves for n_max candidates of at most site_stride sites: the larger of the two shapes the lane
// is promised for, host rows and device-built rows with the reservoir pick, both in the deciding form.  The margins are history
// (16 bytes per shape; 16 more and unrounded move codes + 8 for the built one): they stay because a lent block is never
// regrown and the pinned block's growth rule starts from this value.
template <size_t PairB, size_t RecipB, size_t DecideB>
inline size_t lane_site_buffer_bytes(int n_max, int site_stride) {
    const TrialStaging host = trial_staging<PairB, RecipB, DecideB>(n_max, site_stride, false, false, true);
    const TrialStaging built = trial_staging<PairB, RecipB, DecideB>(n_max, site_stride, true, true, true);
    return std::max(host.total + 16, built.total + 32 + (size_t)n_max * sizeof(int) + 8 - (built.uniforms - built.moves));
}
// The result block, copied out once (offsets in doubles): [split partials of the pair sweep, 2 n_partials | u_old n | u_new n |
// intra n | extra 2 n_pair (the framework part of every pair entry, pair_frozen_kernel; only where some segment has one) |
// accept flags, n ints (deciding form only)]
struct TrialResult {
    size_t partials, u_old, u_new, intra, extra, flags, total;
    size_t flags_bytes() const { return flags * sizeof(double); }
};
inline TrialResult trial_result(int n, int n_partials, int n_pair, bool frozen_extra, bool decide) {
    TrialResult r{};
    r.u_old = 2 * (size_t)n_partials;
    r.u_new = r.u_old + n;
    r.intra = r.u_new + n;
    r.extra = r.intra + n;
    r.flags = r.extra + (frozen_extra ? 2 * (size_t)n_pair : 0);
    r.total = r.flags + (decide ? ((size_t)n + 1) / 2 : 0);
    return r;
}

// ---- The state block of mgpu_state_export_* / mgpu_state_import (mgpu_engine.hip): the whole resident state of n listed
// replicas, the one home of its layout, plain integers as above.  Everything is counted in 8-byte WORDS from the start of the
// block; the values (doubles, and the reservoirs' {count, capacity} int pairs) are copied as words, bit for bit.
//   [head: kStateHeadWords | box: kStateBoxWords | per type {n1, mol_capacity} | per listed replica {replica, A_at} |
//    per (listed replica i, type t) a record of kStateRecWords | data]
// data, replica by replica in the list's order: A(k) (2 n_slots words), then per type
//   pos  3 planes x, y, z of the type's n occupied molecules, each plane in the engine's slot order with the empty slots left
//        out -- plane-major types [site][molecule], site-major ones [molecule][site] -- and padded to an even word count;
//   com  3 planes of nf molecule centres, off 3 planes of nf molecules' offsets (as pos): only where the engine holds frames
//        for the type; nf = n, or 1 where n = 0 and slot 0 still holds the offsets a by-count insertion copies (frames_held);
//   rsv  {count, capacity} (one word), one word of padding, the whole block [capacity][n1][3]: only where there is a reservoir.
// Every segment (A, pos, com, off, rsv) and every plane starts on an even word: 16-byte aligned in the block.
constexpr long long kStateMagic = 0x3141545355504d4dll;      // "MMPUSTA1", little-endian
constexpr int kStateHeadWords = 8;      // magic, n, n_res, n_slots, the engine holds frames (0 / 1), total words, 0, 0
constexpr int kStateBoxWords = 12;      // box matrix (9) and lower bounds (3): the doubles' bit patterns
constexpr int kStateTypeWords = 2, kStateRepWords = 2;
constexpr int kStateRecWords = 8;       // n, nf, reservoir capacity, flags, pos_at, com_at, off_at, rsv_at (-1: none)
enum { kStateRecN, kStateRecNf, kStateRecRsvCap, kStateRecFlags, kStateRecPos, kStateRecCom, kStateRecOff, kStateRecRsv };
// the host-side flags of (replica, type) a later launch reads
enum { kStateInRange = 1, kStateFramesOk = 2, kStateFramesTight = 4, kStateFramesHeld = 8, kStateRsvTight = 16 };
inline size_t state_up2(size_t w) { return (w + 1) & ~(size_t)1; }
inline size_t state_types_at() { return (size_t)kStateHeadWords + kStateBoxWords; }
inline size_t state_reps_at(int n_res) { return state_types_at() + (size_t)kStateTypeWords * n_res; }
inline size_t state_recs_at(int n, int n_res) { return state_reps_at(n_res) + (size_t)kStateRepWords * n; }
inline size_t state_rec_at(int n, int n_res, int i, int t) { return state_recs_at(n, n_res) + (size_t)kStateRecWords * ((size_t)i * n_res + t); }
inline size_t state_data_at(int n, int n_res) { return state_up2(state_rec_at(n, n_res, n, 0)); }
inline size_t state_A_words(int n_slots) { return 2 * (size_t)n_slots; }
inline size_t state_plane_words(int n, int n1) { return state_up2((size_t)n * n1); }      // one plane of n molecules of n1 sites
inline size_t state_rsv_words(int rsv_cap, int n1) { return rsv_cap > 0 ? 2 + state_up2((size_t)3 * rsv_cap * n1) : 0; }
inline int state_frames_held(int n, bool frames_held) { return n > 0 ? n : (frames_held ? 1 : 0); }   // nf
// the segments of one (replica, type) laid out from word `at` on (even); -1: the type has none
struct StateSegs { long long pos, com, off, rsv; size_t end; };
inline StateSegs state_type_segments(size_t at, int n, int nf, int n1, int rsv_cap, bool frames) {
    StateSegs s{-1, -1, -1, -1, at};
    s.pos = (long long)s.end;
    s.end += 3 * state_plane_words(n, n1);
    if (frames) {
        s.com = (long long)s.end;
        s.end += 3 * state_plane_words(nf, 1);
        s.off = (long long)s.end;
        s.end += 3 * state_plane_words(nf, n1);
    }
    if (rsv_cap > 0) {
        s.rsv = (long long)s.end;
        s.end += state_rsv_words(rsv_cap, n1);
    }
    return s;
}
// 16-byte accesses for a run-strided item: block offset, engine offset, run length and run stride all even
inline bool state_item_vec(long long src, long long dst, long long len, long long stride) { return ((src | dst | len | stride) & 1) == 0; }

// ---- The passes of a call over many replicas (mgpu_system_energy_replicas, mgpu_energy_pairs_replicas; mgpu_replicas.hip):
// the listed replicas in the caller's order, per pass as many as `chunk`, a byte budget of scratch and a budget of pair work
// units allow, never fewer than one.
constexpr size_t kReplicasPassBytes = (size_t)256 << 20;       // scratch a pass may take: what bounds the engine's own choice of `chunk`
constexpr int kReplicasPassMax = 32768;                        // replicas per pass (the grids' y extent)
constexpr long long kReplicasPassItems = (long long)1 << 28;   // pair work units (items x splits) per pass
struct Pass { int first, c; long long n_pair, n_in; };
// counts(i, n_pair, n_in): the pair and intra items of list entry i; bytes_of(n_pair, n_in): what such a replica adds to a
// pass.  False (and no passes): one pass's sweep -- a single replica's, past the item budget -- would not fit 2^31 work units
// (less the kWindowPairWaves = kPairWaves a sweep's grid rounds up by); the caller words the refusal.
template <class Counts, class BytesOf>
inline bool plan_passes(int n, Counts counts, BytesOf bytes_of, int chunk, int nsplit, std::vector<Pass> &passes) {
    const int most = chunk > 0 ? std::min(chunk, kReplicasPassMax) : kReplicasPassMax;
    passes.clear();
    for (int i = 0; i < n;) {
        Pass p{i, 0, 0, 0};
        size_t bytes = 0;
        while (i < n && p.c < most) {
            long long np, ni;
            counts(i, np, ni);
            const size_t b = bytes_of(np, ni);
            if (p.c > 0 && (bytes + b > kReplicasPassBytes || (p.n_pair + np) * nsplit > kReplicasPassItems)) break;
            bytes += b; p.n_pair += np; p.n_in += ni; p.c += 1; ++i;
        }
        if (p.n_pair * nsplit >= ((long long)1 << 31) - kWindowPairWaves) { passes.clear(); return false; }
        passes.push_back(p);
    }
    return true;
}

// ---- The accumulators of a farm analysis (mgpu_engine::Rdf, ::Density): one device block of unsigned long long words cut
// into at most three segments; segment s holds per[s] words for every entry (a replica, a group of replicas), entry after
// entry, from word at[s] of the block on.  The read / load / reset calls of every analysis go through this description.
struct Accum {
    int n_seg = 0;
    size_t entries = 0, at[3] = {0, 0, 0}, per[3] = {0, 0, 0}, words = 0;
    size_t word(int s, size_t entry) const { return at[s] + entry * per[s]; }
    size_t bytes() const { return words * sizeof(unsigned long long); }
};
inline Accum accum_layout(size_t entries, size_t per0, size_t per1, size_t per2 = 0) {
    Accum a;
    a.entries = entries;
    for (size_t per : {per0, per1, per2}) {
        if (per == 0) break;
        a.at[a.n_seg] = a.words; a.per[a.n_seg] = per;
        a.words += entries * per; ++a.n_seg;
    }
    return a;
}

// ---- Packed tables of sixteen 4-bit slots in one 64-bit word (RdfTable.row: atom type -> pair index; Density::table: atom
// type -> channel): kNibbleNone marks an empty slot, ~0ull an empty table.
constexpr unsigned kNibbleNone = 0xF;
inline unsigned nibble_get(unsigned long long word, int slot) { return (unsigned)(word >> (4 * slot)) & kNibbleNone; }
inline unsigned long long nibble_set(unsigned long long word, int slot, unsigned v) {
    return (word & ~((unsigned long long)kNibbleNone << (4 * slot))) | ((unsigned long long)v << (4 * slot));
}

}  // namespace mgpu

#endif
