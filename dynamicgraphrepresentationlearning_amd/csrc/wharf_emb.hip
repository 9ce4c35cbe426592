// Queries over an embedding table where it lies: exact top-k
// neighbour search, pair scores, reciprocal row norms, and has_edge for a list.
//
// One score function everywhere: the dot of a pair is the k-ordered f32 chain
// s = fmaf(x[k], y[k], s) from s = 0.  k_emb_score_pairs runs it on the VALU, a
// lane per pair; k_emb_topk runs it on the matrix cores, where
// v_mfma_f32_32x32x2_f32 with its k-steps in ascending order gives the same bits.
//
// Order: a candidate is a 64-bit key, the score's bits made monotone in the high
// word (a zero score as +0) and ~id in the low word, so that "ahead" (score
// descending, id ascending on equal scores) is "greater key", a total order.
// Every selection step is a rank by that key: the result does not depend on
// which lane, wave or block met a candidate first.  No float atomics.
#include <algorithm>
#include <cmath>

#include "wharf_gpu.h"
#include "wharf_kernels.h"

namespace wharf {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr uint32_t kTile = kEmbTile;        // queries of a block, rows of a slab
constexpr uint32_t kPiece = 64;             // columns of a slab staged at a time
constexpr uint32_t kBStride = kPiece + 1;   // floats of a staged row: the 32 lanes of a read group take 32 banks
constexpr uint32_t kWaves = 4;
constexpr unsigned long long kNoCand = kEmbNoCand;

// v in the ascending row adj[off, off + deg)
__device__ __forceinline__ bool row_has(const uint32_t* __restrict__ adj, uint64_t off, uint32_t deg, uint32_t v)
{
    uint32_t lo = 0, hi = deg;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (adj[off + mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo < deg && adj[off + lo] == v;
}

__global__ __launch_bounds__(256) void k_emb_row_norms(const float* __restrict__ emb, uint64_t n, uint32_t dim,
                                                       float* __restrict__ rnorm)
{
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float* x = emb + v * dim;
    const float s = chain_dot(x, x, dim);
    rnorm[v] = s == 0.f ? 0.f : 1.0f / sqrtf(s);
}

__global__ __launch_bounds__(256) void k_emb_score_pairs(const float* __restrict__ emb_q, const float* __restrict__ emb_r,
                                                         const float* __restrict__ rnorm_q,
                                                         const float* __restrict__ rnorm_r,
                                                         const uint32_t* __restrict__ pairs, uint64_t count, uint32_t dim,
                                                         int cosine, float* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint2 p = reinterpret_cast<const uint2*>(pairs)[i];
    float s = chain_dot(emb_q + (uint64_t)p.x * dim, emb_r + (uint64_t)p.y * dim, dim);
    if (cosine) s = (s * rnorm_q[p.x]) * rnorm_r[p.y];
    out[i] = s;
}

__global__ __launch_bounds__(256) void k_has_edges(const uint64_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                                   const uint32_t* __restrict__ adj, const uint32_t* __restrict__ pairs,
                                                   uint64_t count, uint8_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint2 p = reinterpret_cast<const uint2*>(pairs)[i];
    out[i] = row_has(adj, off[p.x], deg[p.x], p.y) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// top-k.  Block: 256 threads = 4 waves; blockIdx.x: a tile of 32 queries (QT tiles, kEmbQueries = 32 QT;
// the sizes below are those of QT = 1, as built), blockIdx.y: the split, rows
// [y n / splits, (y + 1) n / splits).  LDS (dynamic):
//   As   [dim][32]           the queries' rows, k-major: lane l reads A[i = l & 31][k = 2 s + (l >> 5)]
//                            at As[k * 32 + i], 64 consecutive floats of a step
//   Bs   [4][32][65]         a wave's piece (64 columns) of its slab of 32 table rows; the odd stride
//                            puts the 32 lanes of a read group on 32 banks
//   buf  [32][cap] u64       a query's candidates so far, thr [32] u64 its k-th best once it has k,
//   cnt  [32]                pushes (entries beyond cap did not fit and are pushed again after a prune)
//   qid [32], qoff [32] u64, qdeg [32], rq [32]   the query ids, their graph rows, their reciprocal norms
// Wave w takes the slabs w, w + 4, ... of the range; every wave runs the same number of rounds, a
// slab past the range with its row index clamped for the load and its scores discarded.  The next
// piece's 16-B loads are issued before the current piece's 32 MFMA steps.
// ---------------------------------------------------------------------------
template <int DIMW, int QT>
__global__ __launch_bounds__(256) void k_emb_topk(EmbTopkArgs a)
{
    extern __shared__ float4 emb_smem[];
    constexpr uint32_t dim = 64 * DIMW, kQ = kTile * QT;   // kQ: the block's queries, QT tiles of 32
    unsigned long long* buf = reinterpret_cast<unsigned long long*>(emb_smem);
    unsigned long long* thr = buf + kQ * a.cap;
    unsigned long long* qoff = thr + kQ;
    float* As = reinterpret_cast<float*>(qoff + kQ);
    float* Bs = As + dim * kQ;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(Bs + kWaves * kTile * kBStride);
    uint32_t* qid = cnt + kQ;
    uint32_t* qdeg = qid + kQ;
    float* rq = reinterpret_cast<float*>(qdeg + kQ);

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j = lane & 31, h = lane >> 5;
    const uint32_t cap = a.cap, k = a.k;
    const uint64_t q0 = (uint64_t)blockIdx.x * kQ;
    const uint64_t r0 = (uint64_t)blockIdx.y * a.n / a.splits, r1 = ((uint64_t)blockIdx.y + 1) * a.n / a.splits;
    const bool excl_self = a.flags & WHARF_EMB_EXCLUDE_SELF, excl_nb = a.flags & WHARF_EMB_EXCLUDE_NEIGHBOURS;

    if (tid < kQ) {
        const uint64_t qi = q0 + tid < a.q ? q0 + tid : a.q - 1;   // a slot past the list: clamped, never pushed
        const uint32_t v = a.queries[qi];
        qid[tid] = v;
        cnt[tid] = 0;
        thr[tid] = kNoCand;
        rq[tid] = a.cosine ? a.rnorm_q[v] : 1.f;
        qoff[tid] = excl_nb ? a.off[v] : 0;
        qdeg[tid] = excl_nb ? a.deg[v] : 0;
    }
    __syncthreads();
    for (uint32_t idx = tid; idx < kQ * (dim / 4); idx += 256) {
        const uint32_t i = idx % kQ, c = idx / kQ;
        const float4 v = reinterpret_cast<const float4*>(a.emb_q + (uint64_t)qid[i] * dim)[c];
        As[(4 * c + 0) * kQ + i] = v.x;
        As[(4 * c + 1) * kQ + i] = v.y;
        As[(4 * c + 2) * kQ + i] = v.z;
        As[(4 * c + 3) * kQ + i] = v.w;
    }

    const uint64_t slabs = (r1 - r0 + kTile - 1) / kTile, rounds = (slabs + kWaves - 1) / kWaves;
    float* Bw = Bs + wave * kTile * kBStride;
    const uint32_t grow = lane >> 4, gc = lane & 15;   // gather: load g holds chunk gc of the slab's row 4 g + grow
    float4 nxt[8];
    auto gather = [&](uint64_t base, uint32_t piece) {
#pragma unroll
        for (int g = 0; g < 8; g++) {
            uint64_t row = base + 4 * g + grow;
            row = row < a.n ? row : a.n - 1;
            nxt[g] = reinterpret_cast<const float4*>(a.emb_r + row * dim + piece * kPiece)[gc];
        }
    };
    if (rounds) gather(r0 + (uint64_t)wave * kTile, 0);
    __syncthreads();   // As

    for (uint64_t t = 0; t < rounds; t++) {
        const uint64_t base = r0 + (t * kWaves + wave) * kTile;
        const uint64_t row = base + j;
        const bool row_ok = row < r1;
        float rr = 1.f;
        if (a.cosine) rr = a.rnorm_r[row < a.n ? row : a.n - 1];
        f32x16 acc[QT];   // independent chains: one table operand feeds QT query tiles
#pragma unroll
        for (int u = 0; u < QT; u++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[u][r] = 0.f;
#pragma unroll
        for (int piece = 0; piece < DIMW; piece++) {
            // Bw is the wave's own: LDS serves a wave's accesses in issue order, so its stores land after
            // the reads of the piece before and before the reads below; the fences keep the compiler to that order
            wave_lds_order();
#pragma unroll
            for (int g = 0; g < 8; g++) {
                float* o = Bw + (4 * g + grow) * kBStride + 4 * gc;
                o[0] = nxt[g].x;
                o[1] = nxt[g].y;
                o[2] = nxt[g].z;
                o[3] = nxt[g].w;
            }
            if (piece + 1 < DIMW) gather(base, piece + 1);
            else if (t + 1 < rounds) gather(base + kWaves * kTile, 0);
            wave_lds_order();
            const float* ap = As + (piece * kPiece + h) * kQ + j;
            const float* bp = Bw + j * kBStride + h;
#pragma unroll
            for (int s = 0; s < (int)kPiece / 2; s++) {
                const float b = bp[2 * s];
#pragma unroll
                for (int u = 0; u < QT; u++)
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * kQ + kTile * u], b, acc[u], 0, 0, 0);
            }
        }

        // selection: acc[u][r] is the score of table row `row` (the lane's column) and query slot i(u, r)
        unsigned long long key[16 * QT];
        uint32_t pend = 0;
#pragma unroll
        for (int r = 0; r < 16 * QT; r++) {
            const uint32_t i = kTile * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;
            float s = acc[r >> 4][r & 15];
            if (a.cosine) s = (s * rq[i]) * rr;
            key[r] = emb_key(s, (uint32_t)row);
            bool ok = row_ok && q0 + i < a.q && key[r] > thr[i];
            if (ok && excl_self && (uint32_t)row == qid[i]) ok = false;
            if (ok && excl_nb && row_has(a.adj, qoff[i], qdeg[i], (uint32_t)row)) ok = false;
            if (ok) pend |= 1u << r;
        }
        // most rounds of a long scan push nothing: one barrier and on to the next slab
        if (!__syncthreads_or(pend != 0)) continue;
        for (;;) {
#pragma unroll
            for (int r = 0; r < 16 * QT; r++) {
                if (!(pend & (1u << r))) continue;
                const uint32_t i = kTile * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;
                if (key[r] > thr[i]) {
                    const uint32_t pos = atomicAdd(&cnt[i], 1u);   // integer: the set pushed is what matters, not the order
                    if (pos >= cap) continue;                      // full: again after the prune
                    buf[i * cap + pos] = key[r];
                }
                pend &= ~(1u << r);
            }
            __syncthreads();
            // prune (wave w: the queries w, w + 4, ...): keep a query's k best, in order, and raise its threshold
            const uint32_t cl = lane < kQ ? (cnt[lane] < cap ? cnt[lane] : cap) : 0;
            unsigned long long need = __ballot(lane < kQ && (lane & (kWaves - 1)) == wave && cl >= a.prune_at);
            while (need) {
                const uint32_t i = __ffsll((long long)need) - 1;
                need &= need - 1;
                const uint32_t c = __shfl(cl, i);
                unsigned long long* b = buf + i * cap;
                const unsigned long long k0 = lane < c ? b[lane] : kNoCand, k1 = lane + 64 < c ? b[lane + 64] : kNoCand;
                uint32_t rank0 = 0, rank1 = 0;
                for (uint32_t x = 0; x < c; x++) {
                    const unsigned long long kx = b[x];
                    rank0 += kx > k0;
                    rank1 += kx > k1;
                }
                if (lane < c && rank0 < k) b[rank0] = k0;
                if (lane + 64 < c && rank1 < k) b[rank1] = k1;
                if (c >= k) {
                    if (lane < c && rank0 == k - 1) thr[i] = k0;
                    if (lane + 64 < c && rank1 == k - 1) thr[i] = k1;
                }
                if (lane == 0) cnt[i] = c < k ? c : k;
            }
            if (!__syncthreads_or(pend != 0)) break;
        }
    }

    // the block's k best of every query, in order, the tail kNoCand
    __syncthreads();
    for (uint32_t i = wave; i < kQ; i += kWaves) {
        if (q0 + i >= a.q) continue;
        const uint32_t c = cnt[i];   // <= cap: nothing is pending
        const unsigned long long* b = buf + i * cap;
        unsigned long long* out = a.cand + ((uint64_t)blockIdx.y * a.q + q0 + i) * k;
        const unsigned long long k0 = lane < c ? b[lane] : kNoCand, k1 = lane + 64 < c ? b[lane + 64] : kNoCand;
        uint32_t rank0 = 0, rank1 = 0;
        for (uint32_t x = 0; x < c; x++) {
            const unsigned long long kx = b[x];
            rank0 += kx > k0;
            rank1 += kx > k1;
        }
        if (lane < c && rank0 < k) out[rank0] = k0;
        if (lane + 64 < c && rank1 < k) out[rank1] = k1;
        if (lane >= c && lane < k) out[lane] = kNoCand;
    }
}

// A block per query: the k best of its [splits][k] candidates, by rank in the same order.
__global__ __launch_bounds__(256) void k_emb_topk_merge(const unsigned long long* __restrict__ cand, uint64_t q,
                                                        uint32_t k, uint32_t splits, uint32_t* __restrict__ ids,
                                                        float* __restrict__ scores)
{
    __shared__ unsigned long long keys[kEmbMaxSplits * kEmbMaxK];
    __shared__ unsigned long long best[kEmbMaxK];
    const uint64_t qi = blockIdx.x;
    const uint32_t total = splits * k;
    for (uint32_t e = threadIdx.x; e < total; e += 256)
        keys[e] = cand[((uint64_t)(e / k) * q + qi) * k + e % k];
    if (threadIdx.x < k) best[threadIdx.x] = kNoCand;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < total; e += 256) {
        const unsigned long long ke = keys[e];
        if (ke == kNoCand) continue;
        uint32_t rank = 0;
        for (uint32_t x = 0; x < total && rank < k; x++) rank += keys[x] > ke;
        if (rank < k) best[rank] = ke;
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const unsigned long long ke = best[threadIdx.x];
        ids[qi * k + threadIdx.x] = key_id(ke);
        scores[qi * k + threadIdx.x] = key_score(ke);
    }
}

size_t emb_topk_lds(uint32_t dim, uint32_t cap)
{
    constexpr size_t Q = kEmbQueries;
    return Q * cap * 8 + 2 * Q * 8 + ((size_t)dim * Q + kWaves * kTile * kBStride) * 4 + 4 * Q * 4;
}

}  // namespace

uint32_t emb_topk_splits(uint64_t q, uint64_t n)
{
    // about 1024 blocks (a small multiple of 256 CUs), a range no shorter than 4096 rows
    const uint64_t tiles = (q + kEmbQueries - 1) / kEmbQueries;
    uint64_t s = (1024 + tiles - 1) / tiles;
    s = std::min<uint64_t>(s, std::max<uint64_t>(n / 4096, 1));
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(s, 1), kEmbMaxSplits);
}

void launch_emb_row_norms(const float* emb, uint64_t n, uint32_t dim, float* rnorm, hipStream_t s)
{
    hipLaunchKernelGGL(k_emb_row_norms, grid_for(n, 256), 256, 0, s, emb, n, dim, rnorm);
}

void launch_emb_score_pairs(const float* emb_q, const float* emb_r, const float* rnorm_q, const float* rnorm_r,
                            const uint32_t* pairs, uint64_t count, uint32_t dim, int cosine, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_emb_score_pairs, grid_for(count, 256), 256, 0, s, emb_q, emb_r, rnorm_q, rnorm_r, pairs, count,
                       dim, cosine, out);
}

void launch_has_edges(const uint64_t* off, const uint32_t* deg, const uint32_t* adj, const uint32_t* pairs,
                      uint64_t count, uint8_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_has_edges, grid_for(count, 256), 256, 0, s, off, deg, adj, pairs, count, out);
}

void launch_emb_topk(EmbTopkArgs a, uint32_t* ids, float* scores, hipStream_t s)
{
    // more room than k, so that a prune always frees some; small k: a small buffer, two blocks a CU
    a.cap = a.k <= 16 ? 64 : 128;
    a.prune_at = a.k <= 16 ? 48 : 96;
    const size_t lds = emb_topk_lds(a.dim, a.cap);   // up to 98 KB of the CU's 160; dim 128, k <= 16: 66 KB, two blocks a CU
    constexpr int QT = kEmbQueries / kEmbTile;
    const dim3 grid((unsigned)((a.q + kEmbQueries - 1) / kEmbQueries), a.splits);
    switch (a.dim / 64) {
    case 1: hipLaunchKernelGGL((k_emb_topk<1, QT>), grid, 256, lds, s, a); break;
    case 2: hipLaunchKernelGGL((k_emb_topk<2, QT>), grid, 256, lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_emb_topk<3, QT>), grid, 256, lds, s, a); break;
    default: hipLaunchKernelGGL((k_emb_topk<4, QT>), grid, 256, lds, s, a); break;
    }
    hipLaunchKernelGGL(k_emb_topk_merge, (unsigned)a.q, 256, 0, s, a.cand, a.q, a.k, a.splits, ids, scores);
}

}  // namespace wharf
