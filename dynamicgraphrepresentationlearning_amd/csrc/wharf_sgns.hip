// Skip-gram with negative sampling (SGNS) over the resident walk matrix
// (DESIGN.md §10): the noise histogram, the Philox draws of a centre, and the
// trainer that adds into two caller-owned embedding tables in HBM.  Replaces the
// yskip shell-outs of experiments/src/vertex-classification.cpp:142-192.
#include <cmath>
#include <vector>

#include "wharf_gpu.h"
#include "wharf_kernels.h"

namespace wharf {

namespace {

// ---------------------------------------------------------------------------
// noise histogram: count[v] = occurrences of v in the walk matrix (kSent skipped)
// ---------------------------------------------------------------------------
constexpr uint32_t kCountBins = 8192;   // a block's LDS histogram (32 KiB): graphs up to this many vertices

template <bool LDS>
__global__ __launch_bounds__(256) void k_sgns_counts(const uint32_t* __restrict__ walks, uint64_t cells, uint32_t n,
                                                     unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t hist[LDS ? kCountBins : 1];
    if (LDS) {
        for (uint32_t b = threadIdx.x; b < n; b += 256) hist[b] = 0;
        __syncthreads();
    }
    auto put = [&](uint32_t v) {
        if (v >= n) return;   // kSent (and nothing else in a healthy matrix)
        if (LDS) atomicAdd(&hist[v], 1u);
        else atomicAdd(&counts[v], 1ull);
    };
    // the matrix is one contiguous [L][W] array: 16-B loads, consecutive lanes on consecutive quads
    const uint64_t quads = cells / 4, stride = (uint64_t)gridDim.x * 256;
    const uint4* w4 = reinterpret_cast<const uint4*>(walks);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += stride) {
        const uint4 q = w4[i];
        put(q.x); put(q.y); put(q.z); put(q.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < cells - quads * 4) put(walks[quads * 4 + threadIdx.x]);
    if (LDS) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < n; b += 256)
            if (hist[b]) atomicAdd(&counts[b], (unsigned long long)hist[b]);
    }
}

// ---------------------------------------------------------------------------
// listed walk ids -> local columns (ShardMap's inverse; wharf_handle::owned_li)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sgns_columns(const uint32_t* __restrict__ wids, uint64_t count, ShardMap sm,
                                                      uint32_t wpv, uint64_t hi, uint64_t* __restrict__ cols,
                                                      unsigned long long* __restrict__ err)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        const uint64_t wid = wids[i], r = wid / sm.n, v = wid % sm.n;
        bool ok = r < wpv && v >= sm.lo && v < hi;
        uint64_t li = 0;
        if (ok) {
            const uint64_t off = v - sm.lo, q = off >> sm.bits;
            ok = q % sm.parts == sm.part;
            li = r * sm.n_loc + (((q / sm.parts) << sm.bits) | (off & ((1ull << sm.bits) - 1)));
        }
        cols[i] = ok ? li : 0;
        if (!ok) atomicMin(err, (unsigned long long)i);
    }
}

// ---------------------------------------------------------------------------
// the draws of the centre (wid, pos): k_sgns_samples and the trainer both call these
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sgns_window(const SgnsArgs& a, uint64_t wid, uint32_t pos)
{
    const P4 q = philox4x32_10((uint32_t)wid, (uint32_t)(wid >> 32), pos, (a.pass << 4) | kStreamWindow, a.key0, a.key1);
    return 1u + __umulhi(q.x0, a.window);
}

// negative j of the centre (vertex `centre`): kSgnsNone when it equals the centre
__device__ __forceinline__ uint32_t sgns_negative(const SgnsArgs& a, uint64_t wid, uint32_t pos, uint32_t j,
                                                  uint32_t centre)
{
    const P4 q = philox4x32_10((uint32_t)wid, (uint32_t)(wid >> 32), pos | ((j >> 1) << 8),
                               (a.pass << 4) | kStreamNegative, a.key0, a.key1);
    const uint32_t xa = (j & 1) ? q.x2 : q.x0, xb = (j & 1) ? q.x3 : q.x1;
    const uint32_t i = __umulhi(xa, a.n);
    const uint2 e = a.noise[i];
    const uint32_t v = xb < e.x ? i : e.y;
    return v == centre ? kSgnsNone : v;
}

__global__ __launch_bounds__(256) void k_sgns_samples(SgnsArgs a, uint32_t* __restrict__ out)
{
    const uint64_t cells = a.count * a.L;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (uint64_t)gridDim.x * 256) {
        const uint64_t i = c / a.L;
        const uint32_t pos = (uint32_t)(c - i * a.L);
        const uint64_t col = a.cols ? a.cols[i] : i, wid = a.sm.wid(col);
        const uint32_t v = a.walks[(uint64_t)pos * a.W + col];
        uint32_t* o = out + c * (1 + a.K);
        o[0] = v == kSent ? 0u : sgns_window(a, wid, pos);
        for (uint32_t j = 0; j < a.K; j++) o[1 + j] = v == kSent ? kSgnsNone : sgns_negative(a, wid, pos, j, v);
    }
}

// ---------------------------------------------------------------------------
// trainer: one wave per walk; a lane holds elements lane, lane + 64, ... of a row,
// so every row load and every row add is DIMW wave instructions of 256 contiguous bytes
// ---------------------------------------------------------------------------
template <int DIMW>
__device__ __forceinline__ void row_load(const float* p, uint32_t lane, float (&r)[DIMW])
{
    // agent-scope relaxed loads (L2-served): a cached line could predate this wave's own
    // or another CU's atomic adds to the row
#pragma unroll
    for (int j = 0; j < DIMW; j++) r[j] = __hip_atomic_load(p + lane + 64 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int DIMW>
__device__ __forceinline__ void row_add(float* p, uint32_t lane, const float (&r)[DIMW])
{
#pragma unroll
    for (int j = 0; j < DIMW; j++) atomicAdd(p + lane + 64 * j, r[j]);   // result unused: global_atomic_add_f32, no return
}

__device__ __forceinline__ uint32_t walk_at(const uint32_t (&wv)[4], uint32_t q)
{
    const uint32_t x = q < 128 ? (q < 64 ? wv[0] : wv[1]) : (q < 192 ? wv[2] : wv[3]);
    return __builtin_amdgcn_readfirstlane(__shfl(x, q & 63));
}

// One step of the 16-sum reduction: the lanes with BIT set keep values HALF.., the others values
// 0..HALF-1, each summed with its partner's across BIT (compile-time indices: val stays in registers)
template <int HALF, int BIT>
__device__ __forceinline__ void fold(float (&val)[kSgnsMaxTargets], uint32_t lane)
{
    const bool up = lane & BIT;
#pragma unroll
    for (int i = 0; i < HALF; i++) {
        const float send = up ? val[i] : val[i + HALF], keep = up ? val[i + HALF] : val[i];
        val[i] = keep + __shfl_xor(send, BIT);
    }
}

// -log sigma(x) in double
__device__ __forceinline__ double neg_log_sigmoid(double x)
{
    return x >= 0 ? log1p(exp(-x)) : -x + log1p(exp(x));
}

// One walk (column col) by the calling wave.  g: the wave's [2 * kSgnsMaxWindow][kSgnsMaxTargets] LDS floats.
template <int DIMW>
__device__ __forceinline__ void sgns_walk(const SgnsArgs& a, uint64_t col, uint32_t lane, float* g, double& loss,
                                          uint32_t& terms, uint32_t& centres)
{
    const uint64_t wid = a.sm.wid(col);
    uint32_t wv[4];
    uint32_t len = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t p = lane + 64 * i;
        wv[i] = p < a.L ? a.walks[(uint64_t)p * a.W + col] : kSent;
        len += __popcll(__ballot(wv[i] != kSent));   // the walk is a prefix of its column
    }
    const uint32_t myk = lane >> 2;   // the target whose dot product the reduction leaves in this lane
    for (uint32_t pos = 0; pos < len; pos++) {
        if (lane == 0) centres++;
        const uint32_t cv = walk_at(wv, pos);
        const uint32_t b = __builtin_amdgcn_readfirstlane(sgns_window(a, wid, pos));
        const uint32_t q0 = pos > b ? pos - b : 0, q1 = pos + b < len ? pos + b : len - 1;
        if (q1 == q0) continue;   // a walk of one vertex: no context, nothing to add
        // negative j by lane j; targets: bit k of vmask = target k is kept (k = 0: the centre)
        const uint32_t neg = lane < a.K ? sgns_negative(a, wid, pos, lane, cv) : kSgnsNone;
        const uint32_t vmask = 1u | ((uint32_t)__ballot(neg != kSgnsNone) << 1);
        uint32_t tgt[kSgnsMaxTargets];
        float O[kSgnsMaxTargets][DIMW], dO[kSgnsMaxTargets][DIMW];
#pragma unroll
        for (uint32_t k = 0; k < kSgnsMaxTargets; k++) {
            tgt[k] = k ? (uint32_t)__builtin_amdgcn_readlane((int)neg, k ? k - 1 : 0) : cv;
            if ((vmask >> k) & 1) {
                row_load<DIMW>(a.emb_out + (uint64_t)tgt[k] * a.dim, lane, O[k]);
#pragma unroll
                for (int j = 0; j < DIMW; j++) dO[k][j] = 0.f;
            }
        }
        // phase 1: per context, the dot products with every target, g, dO and the loss
        // (context ci sits at position q0 + ci, one further from the centre on; its row is
        // loaded while the context before it is worked on)
        const uint32_t nctx = q1 - q0;
        float hn[DIMW];
        row_load<DIMW>(a.emb_in + (uint64_t)walk_at(wv, q0 + (q0 >= pos)) * a.dim, lane, hn);
        for (uint32_t ci = 0; ci < nctx; ci++) {
            float h[DIMW], val[kSgnsMaxTargets];
#pragma unroll
            for (int j = 0; j < DIMW; j++) h[j] = hn[j];
            if (ci + 1 < nctx) {
                const uint32_t qn = q0 + ci + 1;
                row_load<DIMW>(a.emb_in + (uint64_t)walk_at(wv, qn + (qn >= pos)) * a.dim, lane, hn);
            }
#pragma unroll
            for (uint32_t k = 0; k < kSgnsMaxTargets; k++) {
                float p = 0.f;
                if ((vmask >> k) & 1) {
#pragma unroll
                    for (int j = 0; j < DIMW; j++) p = fmaf(h[j], O[k][j], p);
                }
                val[k] = p;
            }
            // 16 wave sums at once: each step halves the values a lane carries and sums across one
            // lane bit, so 8 + 4 + 2 + 1 + 2 shuffles leave the sum of target (lane >> 2) in every lane
            fold<8, 32>(val, lane);
            fold<4, 16>(val, lane);
            fold<2, 8>(val, lane);
            fold<1, 4>(val, lane);
            float f = val[0];
            f += __shfl_xor(f, 2);
            f += __shfl_xor(f, 1);
            const bool mine = (vmask >> myk) & 1;
            const float label = myk == 0 ? 1.f : 0.f;
            const float gk = mine ? a.lr * (label - 1.f / (1.f + expf(-f))) : 0.f;
            if (mine && (lane & 3) == 0) {
                loss += neg_log_sigmoid(myk == 0 ? (double)f : -(double)f);
                terms++;
                g[ci * kSgnsMaxTargets + myk] = gk;
            }
#pragma unroll
            for (uint32_t k = 0; k < kSgnsMaxTargets; k++) {
                if ((vmask >> k) & 1) {
                    const float gu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gk), 4 * k));
#pragma unroll
                    for (int j = 0; j < DIMW; j++) dO[k][j] = fmaf(gu, h[j], dO[k][j]);
                }
            }
        }
        // lanes 0, 4, ... wrote g, every lane reads it: LDS is in order within a wave, the fence
        // keeps the compiler from moving the reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // phase 2: emb_in[u] += sum_k g_{u,k} O_k (every read of this centre is done)
        for (uint32_t ci = 0; ci < nctx; ci++) {
            const uint32_t q = q0 + ci, u = walk_at(wv, q + (q >= pos));
            float acc[DIMW];
#pragma unroll
            for (int j = 0; j < DIMW; j++) acc[j] = 0.f;
#pragma unroll
            for (uint32_t k = 0; k < kSgnsMaxTargets; k++) {
                if ((vmask >> k) & 1) {
                    const float gu = g[ci * kSgnsMaxTargets + k];
#pragma unroll
                    for (int j = 0; j < DIMW; j++) acc[j] = fmaf(gu, O[k][j], acc[j]);
                }
            }
            row_add<DIMW>(a.emb_in + (uint64_t)u * a.dim, lane, acc);
        }
        // phase 3: emb_out[t_k] += dO_k
#pragma unroll
        for (uint32_t k = 0; k < kSgnsMaxTargets; k++)
            if ((vmask >> k) & 1) row_add<DIMW>(a.emb_out + (uint64_t)tgt[k] * a.dim, lane, dO[k]);
        // the next centre of this walk reads rows this one added to: wait until the adds are done
        // (they execute at the memory side; the loads above are served past L1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // g is rewritten by the next centre
    }
}

// Waves stride over the list: the parallel grid gives every walk a wave of its own (they race:
// Hogwild), the serial grid is one wave that runs the list in order.
template <int DIMW>
__global__ __launch_bounds__(256) void k_sgns_train(SgnsArgs a)
{
    __shared__ float g_all[4][2 * kSgnsMaxWindow * kSgnsMaxTargets];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    double loss = 0;
    uint32_t terms = 0, centres = 0;
    unsigned long long terms_all = 0, centres_all = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * wpb + wave; i < a.count; i += (uint64_t)gridDim.x * wpb) {
        sgns_walk<DIMW>(a, a.cols ? a.cols[i] : i, lane, g_all[wave], loss, terms, centres);
        terms_all += terms;       // a walk: at most 255 * 32 * 16 terms in a lane
        centres_all += centres;
        terms = centres = 0;
    }
    // per wave: one sum in double, one atomic each
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        loss += __shfl_xor(loss, d);
        terms_all += __shfl_xor(terms_all, d);
        centres_all += __shfl_xor(centres_all, d);
    }
    if (lane == 0 && centres_all) {
        atomicAdd(reinterpret_cast<double*>(a.stat), loss);
        atomicAdd(a.stat + 1, terms_all);
        atomicAdd(a.stat + 2, centres_all);
    }
}

}  // namespace

void launch_sgns_counts(const uint32_t* walks, uint64_t cells, uint32_t n, unsigned long long* counts, hipStream_t s)
{
    if (!cells) return;
    const unsigned grid = std::min(grid_for(cells / 4 + 1, 256), cu_count() * 8);
    if (n <= kCountBins) hipLaunchKernelGGL(k_sgns_counts<true>, grid, 256, 0, s, walks, cells, n, counts);
    else hipLaunchKernelGGL(k_sgns_counts<false>, grid, 256, 0, s, walks, cells, n, counts);
}

void launch_sgns_columns(const uint32_t* wids, uint64_t count, const ShardMap& sm, uint32_t wpv, uint64_t hi,
                         uint64_t* cols, unsigned long long* err, hipStream_t s)
{
    if (count) hipLaunchKernelGGL(k_sgns_columns, grid_for(count, 256), 256, 0, s, wids, count, sm, wpv, hi, cols, err);
}

void launch_sgns_samples(const SgnsArgs& a, uint32_t* out, hipStream_t s)
{
    if (a.count) hipLaunchKernelGGL(k_sgns_samples, grid_for(a.count * a.L, 256), 256, 0, s, a, out);
}

void launch_sgns_train(const SgnsArgs& a, bool serial, hipStream_t s)
{
    if (!a.count) return;
    // parallel: 4 waves per block, enough blocks to fill the chip several times over
    const unsigned grid = serial ? 1u : (unsigned)std::min<uint64_t>((a.count + 3) / 4, (uint64_t)cu_count() * 16);
    const unsigned block = serial ? 64u : 256u;
    switch (a.dim / 64) {
    case 1: hipLaunchKernelGGL(k_sgns_train<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_sgns_train<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_sgns_train<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_sgns_train<4>, grid, block, 0, s, a); break;
    }
}

}  // namespace wharf

// ---------------------------------------------------------------------------
// host: the alias table of weights count^power (Vose's method, double precision)
// ---------------------------------------------------------------------------
extern "C" int wharf_sgns_build_alias(const uint64_t* counts, uint64_t n, double power, uint32_t* thr, uint32_t* alias)
{
    if (!counts || !thr || !alias || n == 0 || n >= 0xFFFFFFFEull || !(power >= 0)) return WHARF_E_INVALID;
    std::vector<double> p(n);
    double sum = 0;
    uint64_t best = 0;
    for (uint64_t v = 0; v < n; v++) {
        p[v] = counts[v] ? std::pow((double)counts[v], power) : 0.0;
        sum += p[v];
        if (counts[v] > counts[best]) best = v;
    }
    if (!(sum > 0)) return WHARF_E_INVALID;   // all-zero counts
    // small: p < 1, large: p >= 1, both ascending; the zero-count entries go on top of the
    // small stack, so they are paired while a large entry is sure to exist
    std::vector<uint32_t> small, large;
    for (uint64_t v = 0; v < n; v++) {
        p[v] = p[v] * (double)n / sum;
        if (counts[v] && p[v] < 1.0) small.push_back((uint32_t)v);
        else if (counts[v]) large.push_back((uint32_t)v);
    }
    for (uint64_t v = 0; v < n; v++)
        if (!counts[v]) small.push_back((uint32_t)v);
    auto threshold = [](double q) {
        const double t = std::floor(q * 4294967296.0);
        return t >= 4294967295.0 ? 0xFFFFFFFFu : (t <= 0 ? 0u : (uint32_t)t);
    };
    while (!small.empty() && !large.empty()) {
        const uint32_t s = small.back(), l = large.back();
        small.pop_back();
        large.pop_back();
        thr[s] = threshold(p[s]);
        alias[s] = l;
        p[l] = (p[l] + p[s]) - 1.0;
        (p[l] < 1.0 ? small : large).push_back(l);
    }
    // what is left has p = 1 up to rounding: it aliases itself (a zero-count entry, which
    // rounding alone could leave here, goes to the most frequent vertex instead)
    for (uint32_t v : large) { thr[v] = 0xFFFFFFFFu; alias[v] = v; }
    for (uint32_t v : small) {
        thr[v] = counts[v] ? 0xFFFFFFFFu : 0u;
        alias[v] = counts[v] ? v : (uint32_t)best;
    }
    return WHARF_OK;
}
