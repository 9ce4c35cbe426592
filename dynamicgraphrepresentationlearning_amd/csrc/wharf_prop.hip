// Feature propagation over the graph in HBM: Y = alpha D_l (A + s I) D_r X + beta R,
// the rows of the slack-row CSR as the index of a whole-row gather from the feature table.
//
// A group of G = dim / 4 lanes owns one destination and takes one 16-B load per neighbour row, so a
// wave works on 64 / G destinations at a time (dim 192: one group of 48 lanes, 16 idle).  The group
// walks its row in ascending order and chains the terms with single rounded adds; the loads of kInFlight
// neighbours and the indices of the next kInFlight are issued before the adds of the current ones.
// Rows longer than WHARF_PROP_CHUNK are not walked by their group: the first group that meets such
// a vertex reserves its chunk slots, k_prop_chunks gives every (vertex, chunk) to a group of its own,
// and k_prop_combine adds a row's partials in chunk order.  Every multiply and add is a single
// rounded operation in the order include/wharf_gpu.h states, so the bits are those of the
// sequential restatement whatever the grid, the list or the path of a row.  No float atomics.
#include <algorithm>

#include "wharf_gpu.h"
#include "wharf_kernels.h"

namespace wharf {

namespace {

constexpr uint32_t kChunk = WHARF_PROP_CHUNK;
constexpr int kInFlight = 8;                  // neighbour rows whose loads a lane has in flight
// waves of a block (one against four: within the spread of the probe)
#ifndef WHARF_PROP_WAVES
#define WHARF_PROP_WAVES 4
#endif
constexpr uint32_t kWaves = WHARF_PROP_WAVES, kThreads = 64 * kWaves;
constexpr uint32_t kMaxBlocks = 1u << 22;     // a wave takes the row sets w, w + waves, ...

// HIP's __fadd_rn / __fmul_rn are a plain + and * here, which the compiler contracts into a fused
// multiply-add where one feeds the other (alpha * y + beta * r did).  These two carry no permission
// to contract, whatever -ffp-contract says.
__device__ __forceinline__ float fadd_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ float fmul_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b)
{
    return make_float4(fadd_rn(a.x, b.x), fadd_rn(a.y, b.y), fadd_rn(a.z, b.z), fadd_rn(a.w, b.w));
}

__device__ __forceinline__ float4 mul4(float s, float4 b)
{
    return make_float4(fmul_rn(s, b.x), fmul_rn(s, b.y), fmul_rn(s, b.z), fmul_rn(s, b.w));
}

constexpr int group_width(int g) { return g <= 4 ? 4 : g <= 8 ? 8 : g <= 16 ? 16 : g <= 32 ? 32 : 64; }

// the chain +0 + t_e0 + t_e0+1 + ... over the targets adj[o + e0 .. o + e1) of one row, for the lane's
// four columns.  Nothing is read at or past e1: a lane with e0 == e1 reads nothing at all.
template <int G, bool WS>
__device__ __forceinline__ float4 prop_walk(const PropArgs& a, uint64_t o, uint32_t e0, uint32_t e1, uint32_t gl)
{
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.x);
    const uint32_t* __restrict__ row = a.adj + o;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t u[kInFlight];
#pragma unroll
    for (int j = 0; j < kInFlight; j++) u[j] = e0 + j < e1 ? row[e0 + j] : 0u;
    for (uint32_t e = e0; e < e1; e += kInFlight) {
        float4 t[kInFlight];
        float w[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; j++) {
            t[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            w[j] = 0.f;
            if (e + j < e1) {
                t[j] = x4[(uint64_t)u[j] * G + gl];
                if (WS) w[j] = a.wsrc[u[j]];
            }
        }
        uint32_t un[kInFlight];
#pragma unroll
        for (int j = 0; j < kInFlight; j++) un[j] = e + kInFlight + j < e1 ? row[e + kInFlight + j] : 0u;
#pragma unroll
        for (int j = 0; j < kInFlight; j++) {
            if (e + j < e1) {
                if (WS) t[j] = mul4(w[j], t[j]);
                acc = add4(acc, t[j]);
            }
            u[j] = un[j];
        }
    }
    return acc;
}

// the closing operations of output row i (vertex v) on the row sum A, and the store
template <int G>
__device__ __forceinline__ void prop_finish(const PropArgs& a, float4 A, uint32_t v, uint64_t i, uint32_t gl)
{
    if (a.self) {
        float4 t = reinterpret_cast<const float4*>(a.x)[(uint64_t)v * G + gl];
        if (a.wsrc) t = mul4(a.wsrc[v], t);
        A = add4(A, t);
    }
    if (a.wdst) A = mul4(a.wdst[v], A);
    A = mul4(a.alpha, A);
    if (a.resid) A = add4(A, mul4(a.beta, reinterpret_cast<const float4*>(a.resid)[(uint64_t)v * G + gl]));
    reinterpret_cast<float4*>(a.out)[i * G + gl] = A;
}

// ---------------------------------------------------------------------------
// rows.  Block: kWaves waves; wave w of the grid takes the sets of 64 / GW consecutive output rows
// w, w + waves, ...; group grp of the wave the set's row grp.  A row of at most kChunk targets is
// walked and finished here.  A longer one is left to the two kernels below: lane 0 of the first
// group to meet its vertex reserves nc consecutive chunk slots (slot[v] = the first; items[slot] =
// v for each).  slot[] is all ones on entry; the integer atomics decide only where a partial is
// kept, never a value.
// ---------------------------------------------------------------------------
constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu, kSlotClaimed = 0xFFFFFFFEu;

template <int G, bool WS>
__global__ __launch_bounds__(kThreads) void k_prop_rows(PropArgs a)
{
    constexpr uint32_t GW = group_width(G), GPW = 64 / GW;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (GW - 1), grp = lane / GW;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t rb = ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * GPW; rb < a.rows; rb += waves * GPW) {
        const uint64_t i = rb + grp;
        if (i >= a.rows || gl >= G) continue;
        const uint32_t v = a.vids ? a.vids[i] : (uint32_t)i;
        const uint32_t d = a.deg[v];
        if (d <= kChunk) {
            prop_finish<G>(a, prop_walk<G, WS>(a, a.off[v], 0, d, gl), v, i, gl);
        } else if (gl == 0 && atomicCAS(a.slot + v, kSlotEmpty, kSlotClaimed) == kSlotEmpty) {
            const uint32_t nc = (d + kChunk - 1) / kChunk;
            const uint32_t base = atomicAdd(a.total, nc);
            for (uint32_t c = 0; c < nc; c++) a.items[base + c] = v;
            a.slot[v] = base;
        }
    }
}

// chunks: item t is chunk t - slot[v] of the vertex v = items[t]; a group per item, its partial to part[t]
template <int G, bool WS>
__global__ __launch_bounds__(kThreads) void k_prop_chunks(PropArgs a, uint32_t T)
{
    constexpr uint32_t GW = group_width(G), GPW = 64 / GW;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (GW - 1), grp = lane / GW;
    const uint64_t t = ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * GPW + grp;
    if (t >= T || gl >= G) return;
    const uint32_t v = a.items[t];
    const uint32_t d = a.deg[v], e0 = ((uint32_t)t - a.slot[v]) * kChunk;
    const uint32_t e1 = d - e0 < kChunk ? d : e0 + kChunk;
    reinterpret_cast<float4*>(a.part)[t * G + gl] = prop_walk<G, WS>(a, a.off[v], e0, e1, gl);
}

// combine: the rows k_prop_rows left out, P_0 + P_1 + ... in chunk order, then the closing operations
template <int G>
__global__ __launch_bounds__(kThreads) void k_prop_combine(PropArgs a)
{
    constexpr uint32_t GW = group_width(G), GPW = 64 / GW;
    const uint32_t lane = threadIdx.x & 63, gl = lane & (GW - 1), grp = lane / GW;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves;
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(a.part);
    for (uint64_t rb = ((uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * GPW; rb < a.rows; rb += waves * GPW) {
        const uint64_t i = rb + grp;
        if (i >= a.rows || gl >= G) continue;
        const uint32_t v = a.vids ? a.vids[i] : (uint32_t)i;
        const uint32_t d = a.deg[v];
        if (d <= kChunk) continue;
        const uint32_t nc = (d + kChunk - 1) / kChunk;
        const uint64_t base = a.slot[v];
        float4 A = p4[base * G + gl];
        for (uint32_t c = 1; c < nc; c++) A = add4(A, p4[(base + c) * G + gl]);
        prop_finish<G>(a, A, v, i, gl);
    }
}

unsigned row_blocks(uint64_t rows, uint32_t dim)
{
    const uint32_t gpw = 64 / group_width(dim / 4);
    const uint64_t waves = (rows + gpw - 1) / gpw;
    return (unsigned)std::min<uint64_t>((waves + kWaves - 1) / kWaves, kMaxBlocks);
}

template <bool WS>
void launch_rows(const PropArgs& a, hipStream_t s)
{
    const unsigned blocks = row_blocks(a.rows, a.dim);
    switch (a.dim / 4) {
    case 4: hipLaunchKernelGGL((k_prop_rows<4, WS>), blocks, kThreads, 0, s, a); break;
    case 8: hipLaunchKernelGGL((k_prop_rows<8, WS>), blocks, kThreads, 0, s, a); break;
    case 16: hipLaunchKernelGGL((k_prop_rows<16, WS>), blocks, kThreads, 0, s, a); break;
    case 32: hipLaunchKernelGGL((k_prop_rows<32, WS>), blocks, kThreads, 0, s, a); break;
    case 48: hipLaunchKernelGGL((k_prop_rows<48, WS>), blocks, kThreads, 0, s, a); break;
    default: hipLaunchKernelGGL((k_prop_rows<64, WS>), blocks, kThreads, 0, s, a); break;
    }
}

template <bool WS>
void launch_chunks(const PropArgs& a, uint32_t T, hipStream_t s)
{
    const unsigned blocks = row_blocks(T, a.dim);   // T * dim * 4 bytes of partials exist: far below kMaxBlocks
    switch (a.dim / 4) {
    case 4: hipLaunchKernelGGL((k_prop_chunks<4, WS>), blocks, kThreads, 0, s, a, T); break;
    case 8: hipLaunchKernelGGL((k_prop_chunks<8, WS>), blocks, kThreads, 0, s, a, T); break;
    case 16: hipLaunchKernelGGL((k_prop_chunks<16, WS>), blocks, kThreads, 0, s, a, T); break;
    case 32: hipLaunchKernelGGL((k_prop_chunks<32, WS>), blocks, kThreads, 0, s, a, T); break;
    case 48: hipLaunchKernelGGL((k_prop_chunks<48, WS>), blocks, kThreads, 0, s, a, T); break;
    default: hipLaunchKernelGGL((k_prop_chunks<64, WS>), blocks, kThreads, 0, s, a, T); break;
    }
}

}  // namespace

bool prop_dim_ok(uint32_t dim) { return dim == 16 || dim == 32 || (dim >= 64 && dim <= 256 && dim % 64 == 0); }

uint64_t prop_max_items(uint64_t m)
{
    // a row of d > kChunk targets has ceil(d / kChunk) <= d / 512 + 1 < d / 256 chunks
    return m / 256 + 1;
}

void launch_prop_rows(const PropArgs& a, hipStream_t s)
{
    if (a.wsrc) launch_rows<true>(a, s);
    else launch_rows<false>(a, s);
}

void launch_prop_long(const PropArgs& a, uint32_t T, hipStream_t s)
{
    if (a.wsrc) launch_chunks<true>(a, T, s);
    else launch_chunks<false>(a, T, s);
    const unsigned blocks = row_blocks(a.rows, a.dim);
    switch (a.dim / 4) {
    case 4: hipLaunchKernelGGL(k_prop_combine<4>, blocks, kThreads, 0, s, a); break;
    case 8: hipLaunchKernelGGL(k_prop_combine<8>, blocks, kThreads, 0, s, a); break;
    case 16: hipLaunchKernelGGL(k_prop_combine<16>, blocks, kThreads, 0, s, a); break;
    case 32: hipLaunchKernelGGL(k_prop_combine<32>, blocks, kThreads, 0, s, a); break;
    case 48: hipLaunchKernelGGL(k_prop_combine<48>, blocks, kThreads, 0, s, a); break;
    default: hipLaunchKernelGGL(k_prop_combine<64>, blocks, kThreads, 0, s, a); break;
    }
}

}  // namespace wharf
