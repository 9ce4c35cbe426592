// Softmax-regression vertex classifier over an embedding table where it lies
// (DESIGN.md §11): per-column min/max of the listed rows, the loss / gradient
// pass and the predict / confusion pass.  Replaces the MinMaxScaler +
// LogisticRegression stage of experiments/bin/vertex-classification.py, which the
// reference runs after every yskip run (vertex-classification.cpp:153-194).
//
// One pass works on tiles of kClfRows listed rows.  A tile is gathered with 16-B
// lane loads (the next tile's loads are issued before this tile's arithmetic),
// scaled in registers and stored column-major in LDS, so that the logits and the
// P^T X' product read four rows of a column with one 16-B LDS load.  wb is read
// through L2.  Nothing in a sum is atomic: every block keeps its share of the
// gradient in registers across its tiles, writes it once, and k_clf_reduce adds
// the blocks' shares in block order.
#include <algorithm>
#include <cmath>

#include "wharf_gpu.h"
#include "wharf_kernels.h"

namespace wharf {

namespace {

constexpr uint32_t kRows = kClfRows;        // rows of a tile
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;  // a tile row past the end of the list
constexpr uint32_t kNoElem = 0xFFFFFFFFu;   // an accumulator slot past the block's share of the gradient

// ---------------------------------------------------------------------------
// ids < n, labels < C: the first offending entry of each list (preset to ~0)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clf_check(const uint32_t* __restrict__ vids, const uint32_t* __restrict__ labels,
                                                   uint64_t count, uint64_t n, uint32_t C,
                                                   unsigned long long* __restrict__ err)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        if (vids[i] >= n) atomicMin(err, (unsigned long long)i);
        if (labels && labels[i] >= C) atomicMin(err + 1, (unsigned long long)i);
    }
}

// ---------------------------------------------------------------------------
// per-column min / max of the listed rows: a thread keeps four columns of every
// rs-th row of its block; blocks write [2][dim] each, k_clf_minmax_final folds them
// ---------------------------------------------------------------------------
__device__ __forceinline__ float4 min4(float4 a, float4 b)
{
    return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w));
}
__device__ __forceinline__ float4 max4(float4 a, float4 b)
{
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

__global__ __launch_bounds__(256) void k_clf_minmax(const float* __restrict__ emb, const uint32_t* __restrict__ vids,
                                                    uint64_t count, uint32_t dim, float* __restrict__ part)
{
    __shared__ float4 smn[256], smx[256];
    const uint32_t chunks = dim / 4, rs = 256 / chunks, c4 = threadIdx.x % chunks, sub = threadIdx.x / chunks;
    float4 mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (sub < rs) {
        for (uint64_t i = (uint64_t)blockIdx.x * rs + sub; i < count; i += (uint64_t)gridDim.x * rs) {
            const float4 v = reinterpret_cast<const float4*>(emb + (uint64_t)vids[i] * dim)[c4];
            mn = min4(mn, v);
            mx = max4(mx, v);
        }
    }
    smn[threadIdx.x] = mn;
    smx[threadIdx.x] = mx;
    __syncthreads();
    if (sub == 0) {
        for (uint32_t s = 1; s < rs; s++) {
            mn = min4(mn, smn[s * chunks + c4]);
            mx = max4(mx, smx[s * chunks + c4]);
        }
        float4* o = reinterpret_cast<float4*>(part + (uint64_t)blockIdx.x * 2 * dim);
        o[c4] = mn;
        o[chunks + c4] = mx;
    }
}

__global__ __launch_bounds__(256) void k_clf_minmax_final(const float* __restrict__ part, uint32_t nb, uint32_t dim,
                                                          float* __restrict__ lo, float* __restrict__ hi)
{
    const uint32_t k = threadIdx.x;
    if (k >= dim) return;
    float mn = INFINITY, mx = -INFINITY;
    for (uint32_t b = 0; b < nb; b++) {
        mn = fminf(mn, part[(uint64_t)b * 2 * dim + k]);
        mx = fmaxf(mx, part[(uint64_t)b * 2 * dim + dim + k]);
    }
    lo[k] = mn;
    hi[k] = mx;
}

// ---------------------------------------------------------------------------
// the pass.  Block: 256 threads.  LDS (dynamic):
//   lossr [16] double       a row's -log p_y
//   xs    [dim + 1][16]     the tile's scaled rows, column-major; column dim is 1
//   zs    [C][16]           logits, then exp, then p - onehot
//   red   [16][16], red2 [16][16]   the 16 class parts' max / sum (predict: best value / index) of a row
//   zy    [16]              z_y - max of a row
//   ys    [16]              the rows' labels (kNoLabel past the end of the list)
//   wl    [C][dim + 1]      wb, when it is at most kClfWbLds floats (otherwise wb is read through L2)
// Gather: lane l of wave w holds, of tile row l & 15, the 16-B chunks (l >> 4) + 4 (w + 4 j), j < DIMW.
// Softmax: thread t works on row t & 15 and the classes t >> 4, (t >> 4) + 16, ...
// Gradient: thread t owns the elements t + 256 j, j < ACC, of the block's class tile [c0, c0 + ct).
// ---------------------------------------------------------------------------
template <int DIMW, int ACC, bool PREDICT>
__global__ __launch_bounds__(256) void k_clf_pass(ClfArgs a)
{
    extern __shared__ float4 clf_smem[];
    double* lossr = reinterpret_cast<double*>(clf_smem);
    float* xs = reinterpret_cast<float*>(lossr + kRows);
    float* zs = xs + (a.dim + 1) * kRows;
    float* red = zs + a.C * kRows;
    float* red2 = red + 256;
    float* zy = red2 + 256;
    uint32_t* ys = reinterpret_cast<uint32_t*>(zy + kRows);
    float* wl = reinterpret_cast<float*>(ys + kRows);   // [C][dim + 1] wb, when a.wlds

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = tid & 15, part = tid >> 4;   // softmax / argmax
    const uint32_t rg = lane & 15;                  // gather
    const uint32_t dim = a.dim, C = a.C, dim1 = dim + 1;
    const uint64_t tiles = (a.count + kRows - 1) / kRows;

    uint32_t chunk[DIMW];
    float4 lo4[DIMW], sc4[DIMW], nxt[DIMW];
#pragma unroll
    for (int j = 0; j < DIMW; j++) {
        chunk[j] = (lane >> 4) + 4 * (wave + 4 * j);
        lo4[j] = reinterpret_cast<const float4*>(a.lo)[chunk[j]];
        sc4[j] = reinterpret_cast<const float4*>(a.scale)[chunk[j]];
    }
    auto gather = [&](uint64_t tile) {
        const uint64_t row = tile * kRows + rg;
        const uint32_t vid = row < a.count ? a.vids[row] : a.vids[0];   // a row past the end: its p - onehot is 0
        const float4* p = reinterpret_cast<const float4*>(a.emb + (uint64_t)vid * dim);
#pragma unroll
        for (int j = 0; j < DIMW; j++) nxt[j] = p[chunk[j]];
    };

    // the block's share of the gradient: class tile blockIdx.y
    const uint32_t c0 = blockIdx.y * a.ct, cn = C - c0 < a.ct ? C - c0 : a.ct, E = cn * dim1;
    uint32_t elem[ACC];   // class << 16 | column of the element (kNoElem: none)
    float acc[ACC];
    if (!PREDICT) {
#pragma unroll
        for (int j = 0; j < ACC; j++) {
            const uint32_t e = tid + 256 * j;
            elem[j] = e < E ? ((c0 + e / dim1) << 16) | (e % dim1) : kNoElem;
            acc[j] = 0.f;
        }
    }
    double loss = 0;   // thread 0

    if (tid < kRows) xs[dim * kRows + tid] = 1.f;
    if (a.wlds)
        for (uint32_t i = tid; i < C * dim1; i += 256) wl[i] = a.wb[i];
    uint64_t tile = blockIdx.x;
    if (tile < tiles) gather(tile);
    for (; tile < tiles; tile += gridDim.x) {
        // x' = (x - lo) * scale, a subtract and a multiply
#pragma unroll
        for (int j = 0; j < DIMW; j++) {
            const float4 v = nxt[j];
            float* o = xs + 4 * chunk[j] * kRows + rg;
            o[0] = (v.x - lo4[j].x) * sc4[j].x;
            o[kRows] = (v.y - lo4[j].y) * sc4[j].y;
            o[2 * kRows] = (v.z - lo4[j].z) * sc4[j].z;
            o[3 * kRows] = (v.w - lo4[j].w) * sc4[j].w;
        }
        if (tile + gridDim.x < tiles) gather(tile + gridDim.x);
        if (tid < kRows) {
            const uint64_t row = tile * kRows + tid;
            ys[tid] = row < a.count ? (a.labels ? a.labels[row] : 0u) : kNoLabel;
        }
        __syncthreads();

        // logits, up to 64 classes: a unit is one class and four rows
        auto unit_logits = [&](const float* wsrc) {
            for (uint32_t u = tid; u < 4 * C; u += 256) {
                const uint32_t c = u % C, q = u / C;
                const float* w = wsrc + (uint64_t)c * dim1;
                const float* x = xs + 4 * q;
                float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
                for (uint32_t k = 0; k < dim; k++) {
                    const float wk = w[k];
                    const float4 x4 = *reinterpret_cast<const float4*>(x + k * kRows);
                    z.x = fmaf(wk, x4.x, z.x);
                    z.y = fmaf(wk, x4.y, z.y);
                    z.z = fmaf(wk, x4.z, z.z);
                    z.w = fmaf(wk, x4.w, z.w);
                }
                const float b = w[dim];
                *reinterpret_cast<float4*>(zs + c * kRows + 4 * q) = make_float4(z.x + b, z.y + b, z.z + b, z.w + b);
            }
        };
        // more than 64 classes: a thread takes one class and all 16 rows, so that a weight is loaded once per tile
        auto class_logits = [&](const float* wsrc) {
            for (uint32_t c = tid; c < C; c += 256) {
                const float* w = wsrc + (uint64_t)c * dim1;
                float4 z[4];
#pragma unroll
                for (int q = 0; q < 4; q++) z[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
                for (uint32_t k = 0; k < dim; k++) {
                    const float wk = w[k];
                    const float4* x4 = reinterpret_cast<const float4*>(xs + k * kRows);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float4 x = x4[q];
                        z[q].x = fmaf(wk, x.x, z[q].x);
                        z[q].y = fmaf(wk, x.y, z[q].y);
                        z[q].z = fmaf(wk, x.z, z[q].z);
                        z[q].w = fmaf(wk, x.w, z[q].w);
                    }
                }
                const float b = w[dim];
#pragma unroll
                for (int q = 0; q < 4; q++)
                    reinterpret_cast<float4*>(zs + c * kRows)[q] = make_float4(z[q].x + b, z[q].y + b, z[q].z + b, z[q].w + b);
            }
        };
        // two calls each: the loads of a call are of one address space.  More than 64 classes are more
        // than 4096 gradient elements, so the kernels with ACC = 16 never take the first branch: it is
        // left out of them, and their registers still allow three blocks per CU up to dim 128
        if ((PREDICT || ACC > 16) && C > 64) {
            if (a.wlds) class_logits(wl);
            else class_logits(a.wb);
        } else {
            if (a.wlds) unit_logits(wl);
            else unit_logits(a.wb);
        }
        __syncthreads();

        const uint32_t y = ys[r];
        if (PREDICT) {
            // the lowest class that attains the maximum: ascending within a part, then across the parts
            uint32_t* redi = reinterpret_cast<uint32_t*>(red2);
            if (part < C) {
                float best = zs[part * kRows + r];
                uint32_t bi = part;
                for (uint32_t c = part + 16; c < C; c += 16) {
                    const float z = zs[c * kRows + r];
                    if (z > best) { best = z; bi = c; }
                }
                red[part * kRows + r] = best;
                redi[part * kRows + r] = bi;
            }
            __syncthreads();
            if (part == 0 && y != kNoLabel) {
                float best = red[r];
                uint32_t bi = redi[r];
                const uint32_t parts = C < 16 ? C : 16;
                for (uint32_t p = 1; p < parts; p++) {
                    const float z = red[p * kRows + r];
                    const uint32_t i = redi[p * kRows + r];
                    if (z > best || (z == best && i < bi)) { best = z; bi = i; }
                }
                a.pred[tile * kRows + r] = bi;
                if (a.conf) atomicAdd(a.conf + (uint64_t)y * C + bi, 1ull);   // integer: exact in any order
            }
        } else {
            float m = -INFINITY;
            for (uint32_t c = part; c < C; c += 16) m = fmaxf(m, zs[c * kRows + r]);
            red[part * kRows + r] = m;
            __syncthreads();
            m = red[r];
#pragma unroll
            for (uint32_t p = 1; p < 16; p++) m = fmaxf(m, red[p * kRows + r]);
            float s = 0.f;
            for (uint32_t c = part; c < C; c += 16) {
                const float z = zs[c * kRows + r] - m, e = expf(z);
                zs[c * kRows + r] = e;
                s += e;
                if (c == y) zy[r] = z;
            }
            red2[part * kRows + r] = s;
            __syncthreads();
            s = red2[r];
#pragma unroll
            for (uint32_t p = 1; p < 16; p++) s += red2[p * kRows + r];
            for (uint32_t c = part; c < C; c += 16) {
                const float d = zs[c * kRows + r] / s - (c == y ? 1.f : 0.f);
                zs[c * kRows + r] = y != kNoLabel ? d : 0.f;
            }
            if (part == 0 && y != kNoLabel) lossr[r] = log((double)s) - (double)zy[r];
            __syncthreads();
            if (tid == 0) {
                for (uint32_t i = 0; i < kRows; i++)
                    if (ys[i] != kNoLabel) loss += lossr[i];
            }
            // grad[c][k] += sum over the tile's rows of (p - onehot)[row][c] * x'[row][k], rows in order
#pragma unroll
            for (int j = 0; j < ACC; j++) {
                if (elem[j] == kNoElem) continue;
                const float4* d4 = reinterpret_cast<const float4*>(zs + (elem[j] >> 16) * kRows);
                const float4* x4 = reinterpret_cast<const float4*>(xs + (elem[j] & 0xFFFF) * kRows);
                float g = acc[j];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float4 d = d4[i], x = x4[i];
                    g = fmaf(d.x, x.x, g);
                    g = fmaf(d.y, x.y, g);
                    g = fmaf(d.z, x.z, g);
                    g = fmaf(d.w, x.w, g);
                }
                acc[j] = g;
            }
        }
        __syncthreads();   // the next tile overwrites xs, zs and ys
    }

    if (!PREDICT) {
        float* out = a.partial + (uint64_t)blockIdx.x * C * dim1;
#pragma unroll
        for (int j = 0; j < ACC; j++)
            if (elem[j] != kNoElem) out[(uint64_t)(elem[j] >> 16) * dim1 + (elem[j] & 0xFFFF)] = acc[j];
        if (tid == 0 && blockIdx.y == 0) a.lossp[blockIdx.x] = loss;
    }
}

// ---------------------------------------------------------------------------
// grad[e] = the blocks' shares in block order: 16 groups of consecutive blocks, summed one after
// another each, then the 16 group sums one after another.  The last block does the same for the loss.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clf_reduce(const float* __restrict__ partial, const double* __restrict__ lossp,
                                                    uint32_t nb, uint32_t E, float* __restrict__ grad,
                                                    double* __restrict__ loss_out)
{
    __shared__ float red[16][16];
    __shared__ double dl[256];
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        const uint32_t per = (nb + 255) / 256, b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
        double s = 0;
        for (uint32_t b = b0; b < b1; b++) s += lossp[b];
        dl[tid] = s;
        __syncthreads();
        if (tid == 0) {
            for (uint32_t i = 1; i < 256; i++) s += dl[i];
            *loss_out = s;
        }
        return;
    }
    const uint32_t ge = tid & 15, grp = tid >> 4, e = blockIdx.x * 16 + ge;
    const uint32_t per = (nb + 15) / 16, b0 = grp * per, b1 = b0 + per < nb ? b0 + per : nb;
    float s = 0.f;
    if (e < E)
        for (uint32_t b = b0; b < b1; b++) s += partial[(uint64_t)b * E + e];
    red[grp][ge] = s;
    __syncthreads();
    if (grp == 0 && e < E) {
        for (uint32_t g = 1; g < 16; g++) s += red[g][ge];
        grad[e] = s;
    }
}

size_t clf_lds_bytes(uint32_t dim, uint32_t C, bool wlds)
{
    return kRows * 8 + ((size_t)(dim + 1) * kRows + (size_t)C * kRows + 512 + 2 * kRows + (wlds ? C * (dim + 1) : 0)) * 4;
}

template <int ACC, bool PREDICT>
void launch_pass(ClfArgs a, dim3 grid, hipStream_t s)
{
    a.wlds = a.C * (a.dim + 1) <= kClfWbLds;
    const size_t lds = clf_lds_bytes(a.dim, a.C, a.wlds);
    switch (a.dim / 64) {
    case 1: hipLaunchKernelGGL((k_clf_pass<1, ACC, PREDICT>), grid, 256, lds, s, a); break;
    case 2: hipLaunchKernelGGL((k_clf_pass<2, ACC, PREDICT>), grid, 256, lds, s, a); break;
    case 3: hipLaunchKernelGGL((k_clf_pass<3, ACC, PREDICT>), grid, 256, lds, s, a); break;
    default: hipLaunchKernelGGL((k_clf_pass<4, ACC, PREDICT>), grid, 256, lds, s, a); break;
    }
}

}  // namespace

ClfGrid clf_grid(uint64_t count, uint32_t dim, uint32_t C)
{
    ClfGrid g;
    const uint32_t dim1 = dim + 1;
    // a thread keeps at most 64 gradient elements: beyond 16384 per block the classes are tiled over
    // blockIdx.y (every class tile gathers the rows and computes all logits again)
    g.ct = C * dim1 <= kClfMaxElems ? C : kClfMaxElems / dim1;
    g.tiles_c = (C + g.ct - 1) / g.ct;
    const uint64_t tiles = (count + kClfRows - 1) / kClfRows;
    g.blocks = (uint32_t)std::min<uint64_t>(tiles, std::max(1u, kClfMaxBlocks / g.tiles_c));
    return g;
}

void launch_clf_check(const uint32_t* vids, const uint32_t* labels, uint64_t count, uint64_t n, uint32_t C,
                      unsigned long long* err, hipStream_t s)
{
    hipLaunchKernelGGL(k_clf_check, std::min(grid_for(count, 256), 1024u), 256, 0, s, vids, labels, count, n, C, err);
}

uint32_t clf_minmax_blocks(uint64_t count, uint32_t dim)
{
    const uint32_t rs = 256 / (dim / 4);
    return (uint32_t)std::min<uint64_t>((count + rs - 1) / rs, 512);
}

void launch_clf_minmax(const float* emb, const uint32_t* vids, uint64_t count, uint32_t dim, float* part, float* lo,
                       float* hi, hipStream_t s)
{
    const uint32_t nb = clf_minmax_blocks(count, dim);
    hipLaunchKernelGGL(k_clf_minmax, nb, 256, 0, s, emb, vids, count, dim, part);
    hipLaunchKernelGGL(k_clf_minmax_final, 1, 256, 0, s, part, nb, dim, lo, hi);
}

void launch_clf_loss_grad(const ClfArgs& a, float* grad, double* loss, hipStream_t s)
{
    const ClfGrid g = clf_grid(a.count, a.dim, a.C);
    const dim3 grid(g.blocks, g.tiles_c);
    if (g.ct * (a.dim + 1) <= 16 * 256) launch_pass<16, false>(a, grid, s);
    else launch_pass<64, false>(a, grid, s);
    const uint32_t E = a.C * (a.dim + 1);
    hipLaunchKernelGGL(k_clf_reduce, (E + 15) / 16 + 1, 256, 0, s, a.partial, a.lossp, g.blocks, E, grad, loss);
}

void launch_clf_predict(const ClfArgs& a, hipStream_t s)
{
    const uint64_t tiles = (a.count + kClfRows - 1) / kClfRows;
    launch_pass<1, true>(a, dim3((unsigned)std::min<uint64_t>(tiles, kClfMaxBlocks)), s);
}

}  // namespace wharf
