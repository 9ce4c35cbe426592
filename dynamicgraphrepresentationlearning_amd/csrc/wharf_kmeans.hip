// k-means over an embedding table where it lies, and the statistics of a partition on the
// graph in HBM: the assignment pass, the centroid update, intra-cluster slots
// and volumes.
//
// The score of row i and centroid c is s = chain(x_i, c_c) [* rnorm] - 0.5 chain(c_c, c_c), with
// the k-ordered f32 chain of §12: the row that maximises it is the nearest centroid.  The chain
// runs on the matrix cores (v_mfma_f32_32x32x2_f32, k-steps ascending), which gives the bits of
// the VALU chain.  A candidate is the 64-bit key of §12 (monotone score bits, ~centroid id), the
// assignment the greatest key: the lowest centroid among equal scores, whatever the lane, wave
// or block that met it.  Sums are added in an order fixed by (count, dim, k); no float atomics.
#include <algorithm>
#include <cmath>

#include "wharf_gpu.h"
#include "wharf_kernels.h"

namespace wharf {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr uint32_t kTile = 32;              // the MFMA tile: rows of a wave, centroids of a slab
constexpr uint32_t kPiece = 64;             // columns of a row tile staged at a time
constexpr uint32_t kXStride = kPiece + 1;   // floats of a staged row: the 32 lanes of a read group take 32 banks
constexpr uint32_t kWaves = WHARF_KM_WAVES;   // row tiles of a block, a wave each
constexpr uint32_t kThreads = 64 * kWaves;
constexpr int kSlabLoads = 8 / kWaves;       // 16-B loads of a thread per 64 columns of a slab
constexpr uint32_t kUpdRows = 8;            // update: rows whose loads are in flight together

__global__ __launch_bounds__(256) void k_kmeans_hn(const float* __restrict__ centroids, uint32_t k, uint32_t dim,
                                                   float* __restrict__ hn)
{
    const uint32_t c = threadIdx.x;
    if (c >= k) return;
    const float* x = centroids + (uint64_t)c * dim;
    hn[c] = 0.5f * chain_dot(x, x, dim);
}

// ---------------------------------------------------------------------------
// assign.  Block: 256 threads = 4 waves; a block takes the groups of kKmRows listed rows
// blockIdx.x, blockIdx.x + gridDim.x, ...; wave w the group's rows [32 w, 32 w + 32).  LDS (dynamic):
//   Cs  [dim][32]        a slab of 32 centroids, k-major: lane l reads A[i = l & 31][k = 2 s + (l >> 5)]
//                        at Cs[k * 32 + i], 64 consecutive floats of a step
//   Xs  [4][32][65]      a wave's piece (64 columns) of its 32 rows, gathered through vids with 16-B lane
//                        loads; lane l takes B[k = 2 s + (l >> 5)][j = l & 31] of all dim / 2 steps from it
//                        into registers (XX: and runs the chain x . x of its row over all 64 columns)
//   hs  [256]            0.5 chain(c, c)
//   ds  [4] double       the waves' shares of the group's inertia
// A wave's rows stay in registers across the slabs; every slab is staged once for the four waves, its
// successor's 16-B loads issued before the slab's dim / 2 MFMA steps.  acc[r] is the score of the lane's
// row (column j) and the slab's centroid (r & 3) + 8 (r >> 2) + 4 (l >> 5): a lane keeps the best key of
// its 16, the two half-waves meet in one exchange.  Rows past the list and centroids past k: the index
// clamped for the load, the score discarded.
// ---------------------------------------------------------------------------
template <int DIMW, bool XX>
__global__ __launch_bounds__(kThreads) void k_kmeans_assign(KmArgs a)
{
    extern __shared__ float4 km_smem[];
    constexpr uint32_t dim = 64 * DIMW;
    float* Cs = reinterpret_cast<float*>(km_smem);
    float* Xs = Cs + dim * kTile;
    float* hs = Xs + kWaves * kTile * kXStride;
    double* ds = reinterpret_cast<double*>(hs + kKmMaxK);

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j = lane & 31, h = lane >> 5;
    const uint32_t grow = lane >> 4, gc = lane & 15;   // gather: load g holds chunk gc of the tile's row 4 g + grow
    const uint32_t k = a.k, slabs = (k + kTile - 1) / kTile;
    const uint64_t groups = (a.count + kKmRows - 1) / kKmRows;
    float* Xw = Xs + wave * kTile * kXStride;

    for (uint32_t c = tid; c < k; c += kThreads) hs[c] = a.hn[c];
    double total = 0;   // thread 0

    float4 cn[kSlabLoads * DIMW];   // the next slab: chunk idx >> 5 of its centroid idx & 31, idx = tid + kThreads u
    auto load_slab = [&](uint32_t slab) {
#pragma unroll
        for (int u = 0; u < kSlabLoads * DIMW; u++) {
            const uint32_t idx = tid + kThreads * u, i = idx & 31, c = idx >> 5;
            uint32_t cc = slab * kTile + i;
            cc = cc < k ? cc : k - 1;
            cn[u] = reinterpret_cast<const float4*>(a.centroids + (uint64_t)cc * dim)[c];
        }
    };

    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t base = g * kKmRows + wave * kTile;
        load_slab(0);
        uint32_t vid[8];
#pragma unroll
        for (int gi = 0; gi < 8; gi++) {
            uint64_t ii = base + 4 * gi + grow;
            ii = ii < a.count ? ii : a.count - 1;
            vid[gi] = a.vids ? a.vids[ii] : (uint32_t)ii;
        }
        const uint64_t li = base + j;
        const bool row_ok = li < a.count;
        const uint64_t lic = row_ok ? li : a.count - 1;
        const uint32_t vj = a.vids ? a.vids[lic] : (uint32_t)lic;
        const float rn = a.rnorm ? a.rnorm[vj] : 1.f;

        float4 nx[8];
        auto gather = [&](uint32_t piece) {
#pragma unroll
            for (int gi = 0; gi < 8; gi++)
                nx[gi] = reinterpret_cast<const float4*>(a.emb + (uint64_t)vid[gi] * dim + piece * kPiece)[gc];
        };
        gather(0);
        float xr[32 * DIMW];
        float xx = 0.f;
#pragma unroll
        for (int piece = 0; piece < DIMW; piece++) {
            // Xw is the wave's own: LDS serves a wave's accesses in issue order; the fences keep the compiler to it
            wave_lds_order();
#pragma unroll
            for (int gi = 0; gi < 8; gi++) {
                float* o = Xw + (4 * gi + grow) * kXStride + 4 * gc;
                o[0] = nx[gi].x;
                o[1] = nx[gi].y;
                o[2] = nx[gi].z;
                o[3] = nx[gi].w;
            }
            if (piece + 1 < DIMW) gather(piece + 1);
            wave_lds_order();
            const float* bp = Xw + j * kXStride;
#pragma unroll
            for (int s = 0; s < (int)kPiece / 2; s++) xr[32 * piece + s] = bp[2 * s + h];
            if (XX) {
                // a loop of its own, eight loads at a time: unrolled with the fill it holds 64 more registers
#pragma unroll 8
                for (uint32_t c = 0; c < kPiece; c++) {
                    const float v = bp[c];
                    xx = fmaf(v, v, xx);
                }
            }
        }

        unsigned long long best = 0;   // below the key of every score
        const float* ap = Cs + h * kTile + j;
        for (uint32_t slab = 0; slab < slabs; slab++) {
            __syncthreads();   // the slab before has been read by every wave
#pragma unroll
            for (int u = 0; u < kSlabLoads * DIMW; u++) {
                const uint32_t idx = tid + kThreads * u, i = idx & 31, c = idx >> 5;
                Cs[(4 * c + 0) * kTile + i] = cn[u].x;
                Cs[(4 * c + 1) * kTile + i] = cn[u].y;
                Cs[(4 * c + 2) * kTile + i] = cn[u].z;
                Cs[(4 * c + 3) * kTile + i] = cn[u].w;
            }
            if (slab + 1 < slabs) load_slab(slab + 1);
            __syncthreads();
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < (int)dim / 2; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * kTile], xr[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t c = slab * kTile + (r & 3) + 8 * (r >> 2) + 4 * h;
                float s = acc[r];
                if (a.rnorm) s = __fmul_rn(s, rn);
                s = __fsub_rn(s, hs[c < k ? c : k - 1]);   // a multiply, then a subtract: never fused
                const unsigned long long key = emb_key(s, c);
                if (c < k && key > best) best = key;
            }
        }
        const unsigned long long other = __shfl_xor(best, 32);
        if (other > best) best = other;
        const float sc = key_score(best);
        if (h == 0 && row_ok) {
            a.assign[li] = key_id(best);
            if (a.score) a.score[li] = sc;
        }
        if (XX) {
            // the row's term, then the wave's 32 in a fixed tree, then the four waves in order
            if (a.rnorm) xx = __fmul_rn(__fmul_rn(xx, rn), rn);
            double d = row_ok ? (double)xx - 2.0 * (double)sc : 0.0;
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) d += __shfl_xor(d, m);
            if (lane == 0) ds[wave] = d;
            __syncthreads();   // (the next write of ds is two barriers away)
            if (tid == 0)
                for (uint32_t w = 0; w < kWaves; w++) total += ds[w];
        }
    }
    if (XX && tid == 0) a.part[blockIdx.x] = total;
}

// the blocks' shares in block order: 256 runs of consecutive blocks, summed one after another each,
// then the 256 run sums one after another
__global__ __launch_bounds__(256) void k_kmeans_inertia(const double* __restrict__ part, uint32_t nb,
                                                        double* __restrict__ out)
{
    __shared__ double dl[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (nb + 255) / 256, b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
    double s = 0;
    for (uint32_t b = b0; b < b1; b++) s += part[b];
    dl[tid] = s;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t i = 1; i < 256; i++) s += dl[i];
        *out = s;
    }
}

// ---------------------------------------------------------------------------
// update.  Block: dim threads, thread t the column t; blockIdx.x: the listed rows
// [x count / X, (x + 1) count / X), blockIdx.y: the clusters [y ct, y ct + ct).  LDS (dynamic):
// sums [ct][dim], cnt [ct] (thread 0).  A thread adds its column of every row of the range whose
// cluster is in the tile, in list order, into its own column of sums: no two threads share an
// element, nothing is atomic but the integer counts.  The loads of kUpdRows rows are issued together.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kmeans_update(KmArgs a, const uint32_t* __restrict__ assign, uint32_t ct,
                                                       float* __restrict__ share, unsigned long long* __restrict__ counts)
{
    extern __shared__ float km_sums[];
    const uint32_t t = threadIdx.x, dim = a.dim;
    const uint32_t c0 = blockIdx.y * ct, cn = a.k - c0 < ct ? a.k - c0 : ct;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(km_sums + ct * dim);
    for (uint32_t c = 0; c < cn; c++) km_sums[c * dim + t] = 0.f;
    if (t == 0)
        for (uint32_t c = 0; c < cn; c++) cnt[c] = 0;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.count / gridDim.x, r1 = ((uint64_t)blockIdx.x + 1) * a.count / gridDim.x;
    for (uint64_t i = r0; i < r1; i += kUpdRows) {
        uint32_t cl[kUpdRows];
        float x[kUpdRows];
#pragma unroll
        for (uint32_t u = 0; u < kUpdRows; u++) cl[u] = i + u < r1 ? assign[i + u] - c0 : 0xFFFFFFFFu;   // below c0: wraps past cn
#pragma unroll
        for (uint32_t u = 0; u < kUpdRows; u++) {
            x[u] = 0.f;
            if (cl[u] < cn) {
                const uint32_t v = a.vids ? a.vids[i + u] : (uint32_t)(i + u);
                x[u] = a.emb[(uint64_t)v * dim + t];
                if (a.rnorm) x[u] = __fmul_rn(a.rnorm[v], x[u]);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kUpdRows; u++) {
            if (cl[u] < cn) {
                km_sums[cl[u] * dim + t] = __fadd_rn(km_sums[cl[u] * dim + t], x[u]);
                if (t == 0) cnt[cl[u]]++;
            }
        }
    }
    float* out = share + ((uint64_t)blockIdx.x * a.k + c0) * dim;
    for (uint32_t c = 0; c < cn; c++) out[(uint64_t)c * dim + t] = km_sums[c * dim + t];
    if (t == 0)
        for (uint32_t c = 0; c < cn; c++)
            if (cnt[c]) atomicAdd(counts + c0 + c, (unsigned long long)cnt[c]);   // integer: exact in any order
}

// centroids[e] = (the blocks' shares of element e, one after another in block order) / count; an empty cluster stays
__global__ __launch_bounds__(256) void k_kmeans_reduce(const float* __restrict__ share, uint32_t nb, uint32_t E, uint32_t dim,
                                                       const unsigned long long* __restrict__ counts,
                                                       float* __restrict__ centroids)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const unsigned long long m = counts[e / dim];
    if (!m) return;
    float s = 0.f;
    for (uint32_t b = 0; b < nb; b++) s = __fadd_rn(s, share[(uint64_t)b * E + e]);
    centroids[e] = __fdiv_rn(s, (float)m);
}

// ---------------------------------------------------------------------------
// partition statistics: a wave per vertex u; its lanes walk the row adj[off[u], off[u] + deg[u]) of
// the slack-row CSR and count the targets of u's own part.  Integer atomics: exact in any order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_partition_stats(const uint64_t* __restrict__ off, const uint32_t* __restrict__ deg,
                                                         const uint32_t* __restrict__ adj, const uint32_t* __restrict__ part,
                                                         uint64_t n, unsigned long long* __restrict__ intra,
                                                         unsigned long long* __restrict__ vol)
{
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t u = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < n; u += (uint64_t)gridDim.x * 4) {
        const uint32_t c = part[u], d = deg[u];
        if (!d) continue;
        const uint64_t o = off[u];
        uint32_t hit = 0;
        for (uint32_t e = lane; e < d; e += 64) hit += part[adj[o + e]] == c;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) hit += __shfl_xor(hit, m);
        if (lane == 0) {
            atomicAdd(vol + c, (unsigned long long)d);
            if (hit) atomicAdd(intra + c, (unsigned long long)hit);
        }
    }
}

size_t kmeans_assign_lds(uint32_t dim)
{
    return ((size_t)dim * kTile + kWaves * kTile * kXStride + kKmMaxK) * 4 + kWaves * 8;
}

template <bool XX>
void launch_assign(const KmArgs& a, unsigned blocks, hipStream_t s)
{
    const size_t lds = kmeans_assign_lds(a.dim);   // 42 KB at dim 64 to 67 KB at dim 256
    switch (a.dim / 64) {
    case 1: hipLaunchKernelGGL((k_kmeans_assign<1, XX>), blocks, kThreads, lds, s, a); break;
    case 2: hipLaunchKernelGGL((k_kmeans_assign<2, XX>), blocks, kThreads, lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_kmeans_assign<3, XX>), blocks, kThreads, lds, s, a); break;
    default: hipLaunchKernelGGL((k_kmeans_assign<4, XX>), blocks, kThreads, lds, s, a); break;
    }
}

}  // namespace

uint32_t kmeans_assign_blocks(uint64_t count)
{
    return (uint32_t)std::min<uint64_t>((count + kKmRows - 1) / kKmRows, kKmMaxBlocks);
}

KmUpdGrid kmeans_update_grid(uint64_t count, uint32_t dim, uint32_t k)
{
    KmUpdGrid g;
    g.ct = std::min(k, kKmUpdLds / dim);
    g.tiles_c = (k + g.ct - 1) / g.ct;
    const uint64_t by_share = kKmShareBytes / ((uint64_t)k * dim * 4);
    g.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(count + 63) / 64, kKmUpdMaxBlocks, by_share}));
    return g;
}

void launch_kmeans_hn(const float* centroids, uint32_t k, uint32_t dim, float* hn, hipStream_t s)
{
    hipLaunchKernelGGL(k_kmeans_hn, 1, 256, 0, s, centroids, k, dim, hn);
}

void launch_kmeans_assign(const KmArgs& a, double* inertia, hipStream_t s)
{
    const unsigned blocks = kmeans_assign_blocks(a.count);
    if (a.part) {
        launch_assign<true>(a, blocks, s);
        hipLaunchKernelGGL(k_kmeans_inertia, 1, 256, 0, s, a.part, blocks, inertia);
    } else {
        launch_assign<false>(a, blocks, s);
    }
}

void launch_kmeans_update(const KmArgs& a, const uint32_t* assign, float* share, unsigned long long* counts,
                          float* centroids, hipStream_t s)
{
    const KmUpdGrid g = kmeans_update_grid(a.count, a.dim, a.k);
    const size_t lds = (size_t)g.ct * a.dim * 4 + (size_t)g.ct * 4;
    hipLaunchKernelGGL(k_kmeans_update, dim3(g.blocks, g.tiles_c), a.dim, lds, s, a, assign, g.ct, share, counts);
    const uint32_t E = a.k * a.dim;
    hipLaunchKernelGGL(k_kmeans_reduce, (E + 255) / 256, 256, 0, s, share, g.blocks, E, a.dim, counts, centroids);
}

void launch_partition_stats(const uint64_t* off, const uint32_t* deg, const uint32_t* adj, const uint32_t* part,
                            uint64_t n, unsigned long long* intra, unsigned long long* vol, hipStream_t s)
{
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 3) / 4, 8192);
    hipLaunchKernelGGL(k_partition_stats, blocks, 256, 0, s, off, deg, adj, part, n, intra, vol);
}

}  // namespace wharf
