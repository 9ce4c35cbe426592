// Kernel-side interface of the WharfMH walk engine (shared by the kernels and
// the C-ABI implementation).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "wharf_device.h"

namespace wharf {

enum { kDeepWalk = 0, kNode2Vec = 1 };
enum { kInitRandom = 0, kInitBurnin = 1, kInitWeight = 2 };
constexpr uint64_t kMemoPad = 64;   // >= the chunk of k_rewalk_chunked

struct RunInfo {
    uint64_t off, end;   // old row [off, end)
    uint32_t src, rs, re, pad;
};

struct WalkArgs {
    const ERec* vrec;            // [n]: the row of each vertex
    const ERec* erec;            // [m]: per CSR slot, the target's row (16 B, 32 B with the anchor, or 8 B: rf)
    RecFmt rf;                   // edge-record layout (compact 8-B records: DeepWalk / deterministic)
    const uint32_t* deg;         // [n]: row degrees (a compact record's degree escape)
    const uint32_t* adj;         // [m]: CSR targets (binary searches, anchor proposals)
    uint64_t* anchor;            // node2vec MH: anchor entry of CSR slot e at anchor[e * kAnchorStride]
                                 //   (bytes 16-23 of the slot's 32-B edge record)
    const uint64_t* ehash;       // node2vec: edge hash set (u << 32 | v), or null -> binary search
    uint64_t ehash_mask;         // capacity - 1 (power of two)
    const uint64_t* fdir;        // node2vec MH: per-row neighbour filter {word offset | log2 words << 48}, or null
    const uint32_t* fpool;       //   and its 32-bit words (in front of has_edge in anchor inits)
    uint32_t* walks;             // [L][W]
    const uint64_t* rtab;        // deterministic draws [wpv][L]
    const uint32_t* bitmap;      // batch sources (re-walk)
    const uint32_t* bloom;       // Bloom filter of the batch sources, kBloomWords
    uint8_t* aff;                // per owned walk: re-walk position or kNoRewalk
    unsigned long long* counters;  // [0] steps, [1] accepts, [2] re-walk list, [3..6] WHARF_INIT_STATS, [7] anchor inits
    uint64_t n, n_loc, lo, W;
    uint32_t sh_part, sh_parts, sh_bits;   // the shard's blocks (ShardMap; contiguous: 0, 1, 0)
    uint32_t L, epoch;
    uint32_t key0, key1;
    float inv_p, inv_q;
    int model, init, det;
    int scan_only;               // re-walk: only find rewalk points (apply_walk_updates=false)
    uint64_t* defer;             // node2vec re-walk list {li | p << 56}, tickets << 40 | count in counters[2]
    uint64_t* bdesc;             //   per 256-walk block: its run of the list {offset | count << 40}, or null
    uint64_t* stab;              // node2vec MH re-walk: start-state table, buckets of 4 {key, anchor entry}, or null
    uint64_t stab_mask;          //   buckets - 1
    // deterministic re-walk by suffix table (k_det_suffix + k_rewalk_chunked<true>), or memo == null
    uint32_t* memo;              // [wpv][k][memo_stride]: walk from batch source i in round r, new graph
    const uint32_t* src_idx;     // [n]: index of a batch source in the run table (kNoSource elsewhere when src_exact)
    const RunInfo* runs;         // the batch's source runs
    uint64_t memo_k;             // sources (runs) in the batch
    uint32_t memo_stride;        // L rounded up to 4 (16-B aligned rows)
                                 // (the table has kMemoPad readable words on either side)
    uint32_t wpv;
    int nt_rows;                 // chunked scans: non-temporal walk-matrix row loads (most walks re-walk)
    int park;                    // node2vec MH re-walk by passes (k_rewalk_park / k_park_init), run by the host
    int no_sure;                 // A/B: initialise every uncached anchor a step meets (no sure-accept skip)
    int lane_sort;               // node2vec sorted re-walk: a wave's 64 list entries in column order
    int src_exact;               // src_idx holds kNoSource for every non-source (the copy settles positives by it)
    int ret_first;               // node2vec MH, WEIGHT, 1/p the unique heaviest weight: return-first inits (walk_step)
    unsigned long long* err;     // re-walk list consumers: bit 0 an entry out of range, bit 1 an entry outside its block
    int stage;                   // node2vec re-walk launch: 0 plan + consumer, 1 plan only, 2 consumer only
    int plan_group;              // k_rewalk_plan_lean: bin the 4 blocks of a workgroup together (A/B, no bdesc)
};

__host__ __device__ __forceinline__ ShardMap shard_map(const WalkArgs& a)
{
    return ShardMap{a.n, a.n_loc, a.lo, a.sh_part, a.sh_parts, a.sh_bits};
}

constexpr uint64_t kListMask = (1ull << 40) - 1;   // counters[2]: tickets << 40 | re-walk list entries
constexpr uint64_t kParkRecBytes = 32;   // one parked walker of the node2vec re-walk passes


// per batch source: the new row (slack-row CSR update, k_plan_rows .. k_commit_rows)
constexpr uint64_t kRelocate = ~0ull;   // RowPlan.noff before the merge: the row moves to the pool's end
struct RowPlan {
    uint64_t noff;         // new row start
    uint32_t ndeg, ncap;   // new degree and capacity
    uint32_t ocap, pad;    // old capacity
};

unsigned grid_for(uint64_t work, unsigned block);
unsigned cu_count();

void launch_walk(const WalkArgs& a, bool rewalk, hipStream_t s);
// node2vec MH re-walk passes: fresh = the input is k_rewalk_plan's list, park = walkers that need
// an uncached anchor are appended to `out` instead of initialising it in the wave
void launch_rewalk_park(const WalkArgs& a, int fresh, int park, const void* in, const unsigned long long* in_cnt,
                        void* out, unsigned long long* out_cnt, hipStream_t s);
void launch_park_init(const WalkArgs& a, const void* in, const unsigned long long* in_cnt, hipStream_t s);
void launch_src_index(const RunInfo* runs, uint64_t k, uint32_t* src_idx, hipStream_t s);
void launch_source_degrees(const RunInfo* runs, uint64_t k, const ERec* vrec, uint64_t* out, hipStream_t s);
void launch_anchor_preinit(const WalkArgs& a, const uint64_t* preoff, uint64_t k, hipStream_t s);
void launch_slot_owner_fill(const uint64_t* off, const uint32_t* deg, uint64_t n, uint32_t* owner, hipStream_t s);
// Which order computes a state's anchor up front (round 6, undirected graphs with the reverse-slot
// index): state (cur y, prev x) goes in cur order iff cur's row spans at least t[lg(x)] 128-B lines,
// lg(x) = filt_log2_words(deg x) (the size of prev's neighbour filter).  The host fills t from a
// line-count model (wharf_api.hip, init_order_table); integers, so both kernels decide alike.
constexpr uint32_t kWeightProposals = 21;   // WEIGHT inits: the best of 21 proposals (metropolis_hastings_sampler.h:87-107)
constexpr uint32_t kInitOrderLg = 40;
struct InitOrder {
    uint32_t t[kInitOrderLg];
};
// by_cur_y != 0 (undirected graphs): the states of hub curs (deg > by_cur_y) with small prevs
// (deg <= by_cur_x) computed in cur order by a second kernel (k_anchor_init_by_cur, round 5).
// ridx != null (undirected, reverse-slot index): every state in the cheaper of the two orders by
// `ord` (k_anchor_init_all + k_anchor_init_cur); verify: check each reverse slot before writing.
void launch_anchor_init_all(const WalkArgs& a, const uint32_t* owner, uint64_t slots, uint32_t by_cur_y,
                            uint32_t by_cur_x, const uint32_t* ridx, const InitOrder& ord, bool verify,
                            hipStream_t s);
void launch_vrec(const uint64_t* off, const uint32_t* deg, uint64_t n, const uint32_t* row_epoch, ERec* vrec,
                 hipStream_t s);
void launch_erec(const uint32_t* adj, uint64_t slots, const ERec* vrec, ERec* erec, uint32_t rs, int keep_anchors,
                 RecFmt rf, hipStream_t s);
void launch_rmat_keys(const RmatParams& p, uint64_t M, int directed, uint64_t* keys, hipStream_t s);
void launch_pairs_to_keys(const uint32_t* pairs, uint64_t m, uint64_t n, uint64_t* keys, unsigned long long* err, hipStream_t s);
void launch_csr_to_keys(const uint64_t* off, uint64_t n, const uint32_t* tgt, uint64_t* keys, unsigned long long* err, hipStream_t s);
void launch_unique_flags(const uint64_t* keys, uint64_t m, int drop_loops, uint8_t* keep, hipStream_t s);
void launch_offsets_from_keys(const uint64_t* keys, uint64_t m, uint64_t n, uint64_t* off, hipStream_t s);
void launch_low32(const uint64_t* keys, uint64_t m, uint32_t* out, hipStream_t s);
void launch_batch_change(const uint64_t* bkeys, uint64_t mb, const uint64_t* off, const uint32_t* deg, const uint32_t* adj,
                         int insert, uint32_t* chg, hipStream_t s);
void launch_run_flags(const uint64_t* bkeys, uint64_t mb, uint8_t* f, hipStream_t s);
void launch_run_info(const uint64_t* bkeys, const uint32_t* run_start, uint64_t k, uint64_t mb, const uint64_t* off,
                     const uint32_t* deg, RunInfo* runs, uint32_t* bitmap, uint32_t* bloom, hipStream_t s);
void launch_mark_sources(const uint32_t* src, uint64_t k, RunInfo* runs, uint32_t* bitmap, uint32_t* bloom,
                         hipStream_t s);
void launch_row_degrees(const uint64_t* coff, uint64_t n, uint32_t* deg, uint32_t* cap, uint64_t* capw, int slack,
                        hipStream_t s);
void launch_row_recap(const uint32_t* deg, uint64_t n, uint32_t* cap, uint64_t* capw, int slack, hipStream_t s);
void launch_deg_u64(const uint32_t* deg, uint64_t n, uint64_t* out, hipStream_t s);
void launch_copy_rows(const uint64_t* soff, const uint32_t* deg, const uint32_t* src, const uint64_t* doff, uint64_t n,
                      uint32_t* dst, const uint64_t* sanc, uint64_t* danc, hipStream_t s);
void launch_plan_rows(const RunInfo* runs, uint64_t k, const uint32_t* cap, const uint32_t* cf, int insert, int slack,
                      uint64_t* need, uint64_t* save, RowPlan* plan, unsigned long long* dead, hipStream_t s);
// in-place pool compaction (wharf_handle::compact)
void launch_slot_order_keys(const uint64_t* off, const uint32_t* cap, uint64_t n, uint64_t* keys, uint32_t* vals,
                            hipStream_t s);
void launch_ordered_caps(const uint32_t* order, const uint32_t* cap, uint64_t n, uint64_t* capw, hipStream_t s);
void launch_compact_gather(const uint32_t* order, const uint64_t* snoff, uint64_t r0, uint64_t r1, const uint64_t* off,
                           const uint32_t* deg, const uint32_t* adj, const uint64_t* anc, uint64_t D, uint64_t C,
                           uint32_t* sadj, uint64_t* sanc, hipStream_t s);
void launch_compact_put(const uint32_t* sadj, const uint64_t* sanc, uint64_t cnt, uint64_t D, uint32_t* adj,
                        uint64_t* anc, hipStream_t s);
void launch_scatter_offsets(const uint32_t* order, const uint64_t* snoff, uint64_t n, uint64_t* off, hipStream_t s);
// source rows in chunks (`pre`: exclusive prefix of launch_run_chunks' counts; null: a workgroup per row)
void launch_run_chunks(const RunInfo* runs, const RowPlan* plan, uint64_t k, uint32_t* cnt, hipStream_t s);
void launch_save_rows(const RunInfo* runs, uint64_t k, const uint32_t* pre, const uint32_t* adj, const uint64_t* sofs,
                      uint32_t* scratch, const uint64_t* anc, uint64_t* sanc, const uint32_t* rev, uint32_t* srev,
                      hipStream_t s);
void launch_merge_rows(const RunInfo* runs, uint64_t k, const uint32_t* pre, const uint64_t* bkeys, const uint32_t* chg,
                       const uint32_t* cf, const uint32_t* scratch, const uint64_t* sofs, const uint64_t* relofs,
                       uint64_t pool_end, int insert, RowPlan* plan, uint32_t* adj, const uint64_t* sanc, uint64_t* anc,
                       const uint32_t* srev, uint32_t* rev, hipStream_t s);
void launch_anchor_invalidate(const uint64_t* bkeys, uint64_t mb, const uint32_t* chg, const uint64_t* off,
                              const uint32_t* deg, const uint32_t* adj, uint64_t* anc, const uint64_t* fdir,
                              const uint32_t* fpool, hipStream_t s);
void launch_keys_symmetric(const uint64_t* keys, uint64_t m, unsigned long long* asym, hipStream_t s);
void launch_commit_rows(const RunInfo* runs, uint64_t k, const RowPlan* plan, uint32_t epoch, uint64_t* off,
                        uint32_t* deg, uint32_t* cap, ERec* vrec, uint32_t* row_epoch, hipStream_t s);
void launch_erec_rows(const RunInfo* runs, uint64_t k, const uint32_t* pre, const uint64_t* off, const uint32_t* deg,
                      const uint32_t* adj, const ERec* vrec, ERec* erec, uint32_t rs, int keep_anc, RecFmt rf,
                      hipStream_t s);
void launch_patch_in_edges(const uint32_t* adj, uint64_t slots, const uint32_t* bitmap, const uint32_t* bloom,
                           const ERec* vrec, ERec* erec, uint32_t rs, RecFmt rf, hipStream_t s);
// reverse-slot index (undirected graphs): ridx[e] = the index of x in y's row for slot e = (x -> y)
constexpr uint32_t kNoRidx = 0xFFFFFFFFu;
void launch_rev_build(const uint64_t* off, const uint32_t* deg, const uint32_t* adj, uint64_t n, uint64_t slots,
                      uint32_t* ridx, unsigned long long* miss, hipStream_t s);
void launch_patch_rev(const RunInfo* runs, uint64_t k, const uint32_t* pre, const uint64_t* off, const uint32_t* deg,
                      const uint32_t* adj, const uint32_t* bitmap, const ERec* vrec, ERec* erec, uint32_t rs,
                      RecFmt rf, uint32_t* ridx, unsigned long long* miss, hipStream_t s);
void launch_transpose(const uint32_t* in, uint64_t W, uint32_t L, uint32_t* out, hipStream_t s);
void launch_gather_rows(const uint32_t* walks, uint64_t W, uint32_t L, const uint64_t* list, uint64_t base,
                        uint64_t count, uint32_t* out, hipStream_t s);
void launch_walk_lengths(const uint32_t* walks, uint64_t W, uint32_t L, uint32_t v0, uint32_t v1, uint64_t* len,
                         hipStream_t s);
void launch_index_entries(const uint32_t* walks, uint64_t W, uint32_t L, const ShardMap& sm, int kb,
                          uint32_t v0, uint32_t v1, const uint64_t* col_base, uint64_t* skeys, uint32_t* vals,
                          hipStream_t s);
void launch_index_split(const uint64_t* skeys, uint64_t E, int kb, unsigned long long* counts, uint64_t* keys,
                        hipStream_t s);
unsigned aff_blocks(uint64_t W);
void launch_aff_count(const uint8_t* aff, uint64_t W, uint32_t* counts, hipStream_t s);
void launch_aff_write(const uint8_t* aff, uint64_t W, const uint32_t* offs, const ShardMap& sm,
                      uint32_t* out, hipStream_t s);
void launch_index_pair(const uint64_t* keys, const uint32_t* nexts, uint64_t E, uint64_t* out, hipStream_t s);
void launch_rel_offsets(const uint64_t* off, uint64_t v0, uint64_t cnt, uint32_t* rel, hipStream_t s);
void launch_fill_u32(uint32_t* p, uint64_t cnt, uint32_t v, hipStream_t s);
void launch_fill_u64(uint64_t* p, uint64_t cnt, uint64_t v, hipStream_t s);
void launch_edge_hash_update(const uint64_t* bkeys, uint64_t mb, const uint32_t* chg, int insert, uint64_t* table,
                             uint64_t mask, hipStream_t s);
void launch_edge_hash_build(const uint64_t* off, const uint32_t* deg, uint64_t n, const uint32_t* adj, uint64_t* table,
                            uint64_t mask, hipStream_t s);
void launch_filter_sizes(const uint32_t* deg, uint64_t n, uint64_t* words, hipStream_t s);
void launch_filter_pack(const uint32_t* deg, uint64_t n, uint64_t* fdir, hipStream_t s);
void launch_filter_fill(const uint64_t* off, const uint32_t* deg, uint64_t n, const uint32_t* adj, const uint64_t* fdir,
                        uint32_t* pool, hipStream_t s);
void launch_filter_plan(const RunInfo* runs, uint64_t k, const uint32_t* deg, const uint64_t* fdir, uint64_t* need,
                        hipStream_t s);
void launch_filter_rows(const RunInfo* runs, uint64_t k, const uint32_t* pre, const uint64_t* noff, const uint32_t* deg,
                        const uint32_t* adj, const uint64_t* need, const uint64_t* gofs, uint64_t base, uint64_t* fdir,
                        uint32_t* pool, hipStream_t s);
void launch_szudzik64(int op, uint64_t cnt, uint64_t* x, uint64_t* y, uint64_t* z, hipStream_t s);

// skip-gram with negative sampling over the walk matrix (wharf_sgns.hip)
constexpr uint32_t kSgnsNone = 0xFFFFFFFFu;        // a dropped negative (equal to the centre)
constexpr uint32_t kSgnsMaxTargets = 16;           // the centre + at most 15 negatives
constexpr uint32_t kSgnsMaxWindow = 16;
constexpr uint64_t kSgnsSerialCap = 1ull << 20;    // positions one serial call may cover
struct SgnsArgs {
    const uint32_t* walks;       // [L][W]
    uint64_t W;
    uint32_t L;
    ShardMap sm;
    const uint64_t* cols;        // the listed walks' columns, or null: column i
    uint64_t count;
    const uint2* noise;          // [n] alias table {thr, alias} (unused when K == 0)
    uint32_t n;
    uint32_t key0, key1, pass, window, K, dim;
    float lr;
    float* emb_in;               // [n][dim]
    float* emb_out;              // [n][dim]
    unsigned long long* stat;    // [0] loss (double), [1] terms, [2] centres
};
void launch_sgns_counts(const uint32_t* walks, uint64_t cells, uint32_t n, unsigned long long* counts, hipStream_t s);
// wid -> column for a device id list; *err (preset to ~0) = the first entry that is not owned
void launch_sgns_columns(const uint32_t* wids, uint64_t count, const ShardMap& sm, uint32_t wpv, uint64_t hi,
                         uint64_t* cols, unsigned long long* err, hipStream_t s);
void launch_sgns_samples(const SgnsArgs& a, uint32_t* out, hipStream_t s);
void launch_sgns_train(const SgnsArgs& a, bool serial, hipStream_t s);

// softmax-regression classifier over an embedding table (wharf_clf.hip)
constexpr uint32_t kClfRows = 16;            // listed rows of a tile
constexpr uint32_t kClfMaxElems = 16384;     // gradient elements a block keeps in registers (64 per thread)
constexpr uint32_t kClfWbLds = 6144;         // wb of at most this many floats is staged in LDS by every block
// blocks of a pass: a constant, so the grid does not depend on the device (256 CUs x 2 or 3 resident blocks divide it)
constexpr uint32_t kClfMaxBlocks = 1536;
struct ClfArgs {
    const float* emb;            // [n][dim]
    const uint32_t* vids;        // [count] rows to use
    const uint32_t* labels;      // [count], or null (predict without a confusion matrix)
    uint64_t count;
    uint32_t dim, C, ct;         // ct: classes of a block's share of the gradient
    uint32_t wlds;               // set by the launcher: wb is staged in LDS
    const float* lo;             // [dim]
    const float* scale;          // [dim]
    const float* wb;             // [C][dim + 1]
    float* partial;              // [blocks][C][dim + 1] the blocks' shares of the gradient
    double* lossp;               // [blocks] the blocks' shares of the loss
    uint32_t* pred;              // [count] (predict)
    unsigned long long* conf;    // [C][C], or null (predict)
};
struct ClfGrid {
    uint32_t blocks, tiles_c, ct;   // gridDim.x, gridDim.y, classes per class tile
};
ClfGrid clf_grid(uint64_t count, uint32_t dim, uint32_t C);   // a function of (count, dim, C) alone
uint32_t clf_minmax_blocks(uint64_t count, uint32_t dim);
// *err, err[1] (preset to ~0) = the first id >= n, the first label >= C (labels may be null)
void launch_clf_check(const uint32_t* vids, const uint32_t* labels, uint64_t count, uint64_t n, uint32_t C,
                      unsigned long long* err, hipStream_t s);
// part: [clf_minmax_blocks][2][dim] floats
void launch_clf_minmax(const float* emb, const uint32_t* vids, uint64_t count, uint32_t dim, float* part, float* lo,
                       float* hi, hipStream_t s);
void launch_clf_loss_grad(const ClfArgs& a, float* grad, double* loss, hipStream_t s);
void launch_clf_predict(const ClfArgs& a, hipStream_t s);

// queries over an embedding table (wharf_emb.hip)
constexpr uint32_t kEmbTile = 32;            // the MFMA tile: table rows of a slab, queries of a query tile
// queries of a block: one tile.  Two tiles fed by one table operand (64) halve the bytes streamed, but
// their registers and LDS leave one block a CU: 23.5 ms against 16.9 ms on the probe shape
constexpr uint32_t kEmbQueries = 32;
constexpr uint32_t kEmbMaxK = 64;
constexpr uint32_t kEmbMaxSplits = 64;
// a candidate: monotone score bits << 32 | ~id, greater = ahead; this one is {0xFFFFFFFF, -inf}, behind every row
constexpr unsigned long long kEmbNoCand = 0x007FFFFFull << 32;
struct EmbTopkArgs {
    const float* emb_q;          // [n][dim]
    const float* emb_r;          // [n][dim]
    const float* rnorm_q;        // [n] (cosine)
    const float* rnorm_r;        // [n] (cosine)
    const uint32_t* queries;     // [q]
    uint64_t q, n;
    uint32_t dim, k, flags, splits, cosine;
    uint32_t cap, prune_at;      // set by the launcher: a query's candidate buffer in LDS, the fill that prunes it
    const uint64_t* off;         // the slack-row CSR (WHARF_EMB_EXCLUDE_NEIGHBOURS)
    const uint32_t* deg;
    const uint32_t* adj;
    unsigned long long* cand;    // [splits][q][k] the blocks' candidates, in order
};
uint32_t emb_topk_splits(uint64_t q, uint64_t n);   // splits == 0: a function of (q, n) alone
void launch_emb_row_norms(const float* emb, uint64_t n, uint32_t dim, float* rnorm, hipStream_t s);
void launch_emb_score_pairs(const float* emb_q, const float* emb_r, const float* rnorm_q, const float* rnorm_r,
                            const uint32_t* pairs, uint64_t count, uint32_t dim, int cosine, float* out, hipStream_t s);
void launch_emb_topk(EmbTopkArgs a, uint32_t* ids, float* scores, hipStream_t s);
void launch_has_edges(const uint64_t* off, const uint32_t* deg, const uint32_t* adj, const uint32_t* pairs,
                      uint64_t count, uint8_t* out, hipStream_t s);

// k-means over an embedding table, partition statistics of the graph (wharf_kmeans.hip)
constexpr uint32_t kKmMaxK = 256;
// listed rows of a block's group: four 32-row tiles, one per wave, fed by one staged slab of 32 centroids
// (one tile a block: 1.29 times the time at k = 256 on the probe shape, two: 1.02)
#ifndef WHARF_KM_WAVES
#define WHARF_KM_WAVES 4
#endif
static_assert(WHARF_KM_WAVES == 1 || WHARF_KM_WAVES == 2 || WHARF_KM_WAVES == 4,
              "k_kmeans_assign deals a slab's 16-B loads over 64, 128 or 256 threads");
constexpr uint32_t kKmRows = 32 * WHARF_KM_WAVES;
constexpr uint32_t kKmMaxBlocks = 16384;         // assign: blocks at most (a block takes the groups b, b + blocks, ...)
constexpr uint32_t kKmUpdLds = 8192;             // update: floats of a block's [cluster tile][dim] sums (32 KB)
constexpr uint32_t kKmUpdMaxBlocks = 2048;       // update: row ranges at most
constexpr size_t kKmShareBytes = 64ull << 20;    // update: the blocks' shares [blocks][k][dim], at most
struct KmArgs {
    const float* emb;            // [n][dim]
    const float* rnorm;          // [n], or null
    const uint32_t* vids;        // [count], or null: rows 0..count-1
    uint64_t count;
    uint32_t dim, k;
    const float* centroids;      // [k][dim]
    const float* hn;             // [k] 0.5 chain(c, c)
    uint32_t* assign;            // [count]
    float* score;                // [count], or null
    double* part;                // [blocks] the blocks' shares of the inertia, or null
};
struct KmUpdGrid {
    uint32_t blocks, tiles_c, ct;   // gridDim.x (row ranges), gridDim.y, clusters per cluster tile
};
uint32_t kmeans_assign_blocks(uint64_t count);                   // a function of count alone
KmUpdGrid kmeans_update_grid(uint64_t count, uint32_t dim, uint32_t k);   // a function of (count, dim, k) alone
void launch_kmeans_hn(const float* centroids, uint32_t k, uint32_t dim, float* hn, hipStream_t s);
// inertia: a device double, written when a.part is given
void launch_kmeans_assign(const KmArgs& a, double* inertia, hipStream_t s);
// share: [blocks][k][dim] floats; counts: [k] u64, zeroed by the caller; centroids are updated in place
void launch_kmeans_update(const KmArgs& a, const uint32_t* assign, float* share, unsigned long long* counts,
                          float* centroids, hipStream_t s);
// intra, vol: [k] u64, zeroed by the caller
void launch_partition_stats(const uint64_t* off, const uint32_t* deg, const uint32_t* adj, const uint32_t* part,
                            uint64_t n, unsigned long long* intra, unsigned long long* vol, hipStream_t s);

// feature propagation over the graph (wharf_prop.hip)
struct PropArgs {
    const uint64_t* off;         // the slack-row CSR: row v is adj[off[v], off[v] + deg[v]), ascending
    const uint32_t* deg;
    const uint32_t* adj;
    const float* x;              // [n][dim]
    const float* wsrc;           // [n], or null
    const float* wdst;           // [n], or null
    const float* resid;          // [n][dim], or null
    const uint32_t* vids;        // [rows], or null: rows 0..rows-1
    uint64_t rows;
    uint32_t dim, self;
    float alpha, beta;
    float* out;                  // [rows][dim]
    uint32_t* slot;              // [n] all ones on entry; the first chunk slot of a vertex with a long row
    uint32_t* items;             // [prop_max_items(m)] the vertex of every reserved chunk slot
    uint32_t* total;             // zero on entry; the chunk slots reserved
    float* part;                 // [total][dim] the chunk partials (launch_prop_long)
};
bool prop_dim_ok(uint32_t dim);
uint64_t prop_max_items(uint64_t m);   // chunk slots at most, m the stored targets of the graph
// every row of at most WHARF_PROP_CHUNK targets, and the reservation of the others' chunk slots
void launch_prop_rows(const PropArgs& a, hipStream_t s);
// the other rows: T = *total chunk partials, then their sums in chunk order
void launch_prop_long(const PropArgs& a, uint32_t T, hipStream_t s);

}  // namespace wharf
