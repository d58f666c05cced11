// Block vector algebra on the padded stencil layout: the Gram matrix of two lists of
// vectors and linear combinations of a list of vectors, each as one streaming pass
// (poms_block_gram / poms_block_combine; poms_amd.eigen's LOBPCG).
//
// Both run over the flat range of the vector kernels (vec_ops.hip: whole interior planes;
// the ghost rows / columns and dead pitch columns inside it are zero in every vector, add
// nothing to a sum and are mapped to zero by a linear combination).  The pointer lists
// are kernel arguments, passed by value: no device pointer table, nothing allocated.
// HBM-bound: 16-B accesses where every pointer of the call has the same 16-B phase (a
// leading / trailing single element by one thread, as vec_flat_kernel), 8-B otherwise.
#include "common.hpp"
#include "launchers.hpp"

#include <type_traits>

namespace poms {

typedef double d2 __attribute__((ext_vector_type(2)));

// ---- Gram: G[i][j] = sum_e x_i[e] y_j[e] -------------------------------------------
// The output is cut into kGramTile x kGramTile tiles; blockIdx.y is the tile, blockIdx.x
// a grid-stride walk over the range.  A thread holds the tile's 16 sums in registers and
// loads each of its 4 + 4 vectors once per element: a pass of the n x n Gram matrix reads
// (n/T)^2 2T = 2 n^2 / T vectors (n (n/T + 1) of a symmetric one) where pairwise dots read
// 2 n^2 (n (n + 1)).  The blocks per tile are few (gram_blocks: about 2048 in all), each a
// long grid-stride walk; at 3 waves per SIMD about 768 of them are resident, so two or
// three tiles of a 12 x 12 call walk the range at a time and the others follow: tiles
// that share a vector may find it in the L2 / Infinity Cache, which nothing here relies on.
// Per-block sums go to partial[(t * 16 + e) * nblk + blk]; gram_reduce_kernel adds them
// in a fixed order: no atomics, the same bits every call.
struct GramArgs {
    const double* x[kBlockMax];
    const double* y[kBlockMax];
    int nx, ny, ny_out;
    unsigned char ti[kGramMaxTiles], tj[kGramMaxTiles];   // the launch's tiles (symmetric: tj >= ti)
};

template <bool VEC>
__global__ void __launch_bounds__(256)   // (134 VGPRs: 3 waves per SIMD; a bound of 4 spills)
block_gram_kernel(const GramArgs a, const int head, const int64_t n, const int tail, double* __restrict__ partial) {
    constexpr int T = kGramTile, U = 2;
    using E = std::conditional_t<VEC, d2, double>;
    __shared__ double red[4][T * T];
    const int t = blockIdx.y;
    const int i0 = a.ti[t] * T, j0 = a.tj[t] * T;
    // a ragged tile edge repeats its last vector (the sums of the repeats are dropped)
    const double *xp[T], *yp[T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        xp[k] = a.x[min(i0 + k, a.nx - 1)];
        yp[k] = a.y[min(j0 + k, a.ny - 1)];
    }
    double s[T][T];
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) s[p][q] = 0.0;
    const int64_t step = (int64_t)gridDim.x * 256 * U;
    for (int64_t base = (int64_t)blockIdx.x * 256 * U + threadIdx.x; base < n; base += step) {
        E xv[U][T], yv[U][T];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * 256;
            if (i < n) {
#pragma unroll
                for (int k = 0; k < T; ++k) {
                    xv[u][k] = __builtin_nontemporal_load((const E*)(xp[k] + head) + i);
                    yv[u][k] = __builtin_nontemporal_load((const E*)(yp[k] + head) + i);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + u * 256;
            if (i < n) {
#pragma unroll
                for (int p = 0; p < T; ++p)
#pragma unroll
                    for (int q = 0; q < T; ++q) {
                        if constexpr (VEC) {
                            s[p][q] = fma(xv[u][p].x, yv[u][q].x, s[p][q]);
                            s[p][q] = fma(xv[u][p].y, yv[u][q].y, s[p][q]);
                        } else {
                            s[p][q] = fma(xv[u][p], yv[u][q], s[p][q]);
                        }
                    }
            }
        }
    }
    if constexpr (VEC) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (int e = 0; e < 2; ++e) {
                if (!(e == 0 ? head : tail)) continue;
                const int64_t o = e == 0 ? 0 : head + 2 * n;
#pragma unroll
                for (int p = 0; p < T; ++p)
#pragma unroll
                    for (int q = 0; q < T; ++q) s[p][q] = fma(xp[p][o], yp[q][o], s[p][q]);
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = 0; q < T; ++q) {
            double v = s[p][q];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) red[wv][p * T + q] = v;
        }
    __syncthreads();
    if (threadIdx.x < T * T) {
        const int e = threadIdx.x;
        partial[((int64_t)t * (T * T) + e) * gridDim.x + blockIdx.x] =
            (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    }
}

// One wave per tile entry: a strided running sum of the entry's nblk partials per lane, then
// the wave butterfly.  A symmetric call's entry (i, j), j >= i, is stored at (j, i) too.
__global__ void __launch_bounds__(256)
gram_reduce_kernel(const GramArgs a, const int ntiles, const int nblk, const int symmetric,
                   const double* __restrict__ partial, double* __restrict__ out) {
    constexpr int T = kGramTile;
    const int lane = threadIdx.x & 63;
    const int ent = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ent >= ntiles * T * T) return;
    const int t = ent / (T * T), e = ent - t * (T * T);
    const int i = a.ti[t] * T + e / T, j = a.tj[t] * T + e % T;
    if (i >= a.nx || j >= a.ny || (symmetric && j < i)) return;
    const double* pe = partial + (int64_t)ent * nblk;
    double s = 0.0;
    for (int k = lane; k < nblk; k += 64) s += pe[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        out[(int64_t)i * a.ny_out + j] = s;
        if (symmetric && j > i) out[(int64_t)j * a.ny_out + i] = s;
    }
}

// Blocks per tile: a function of the range and of (nx, ny) alone -- not of `symmetric`, so
// the entries a symmetric call computes have the bits of the full call's -- such that all
// the tiles together are about 2048 blocks and their partials fit the scratch.
static int gram_blocks(int64_t n, int nx, int ny) {
    const int tiles = ((nx + kGramTile - 1) / kGramTile) * ((ny + kGramTile - 1) / kGramTile);
    int64_t cap = 2048 / tiles;
    cap = cap < 64 ? 64 : cap > 512 ? 512 : cap;
    int64_t nb = (n + 256 * 2 - 1) / (256 * 2);
    nb = nb < 1 ? 1 : nb > cap ? cap : nb;
    return (int)nb;
}
static_assert(kGramMaxTiles * 64 * kGramTile * kGramTile <= kScratch &&
                  2048 * kGramTile * kGramTile <= kScratch,
              "the Gram kernel's partials (tiles x blocks x tile entries) must fit the context scratch");

// 16-B phase shared by all of `ptrs`: 0 or 8 (bytes), or -1 if they differ
static int common_phase(const double* const* ptrs, int n, int phase) {
    for (int k = 0; k < n; ++k) {
        const int m = (int)(reinterpret_cast<uintptr_t>(ptrs[k]) & 15);
        if (phase == -2) phase = m;
        if (m != phase) return -1;
    }
    return phase;
}

int block_gram_launch(int64_t count, int nx, const double* const* xs, int ny, const double* const* ys,
                      int symmetric, double* partial, double* out, hipStream_t st) {
    if (nx < 1 || ny < 1 || nx > kBlockMax || ny > kBlockMax || count < 1 || (symmetric && nx != ny)) return 1;
    GramArgs a{};
    for (int k = 0; k < kBlockMax; ++k) {
        a.x[k] = xs[k < nx ? k : 0];
        a.y[k] = ys[k < ny ? k : 0];
    }
    a.nx = nx;
    a.ny = a.ny_out = ny;
    const int tx = (nx + kGramTile - 1) / kGramTile, ty = (ny + kGramTile - 1) / kGramTile;
    int nt = 0;
    for (int i = 0; i < tx; ++i)
        for (int j = symmetric ? i : 0; j < ty; ++j) {
            a.ti[nt] = (unsigned char)i;
            a.tj[nt] = (unsigned char)j;
            ++nt;
        }
    int phase = common_phase(xs, nx, -2);
    if (phase >= 0) phase = common_phase(ys, ny, phase);
    const bool vec = phase >= 0 && count >= 4;
    const int head = vec && phase ? 1 : 0;
    const int64_t n = vec ? (count - head) / 2 : count;
    const int tail = vec ? (int)((count - head) - 2 * n) : 0;
    // (the grid from the range in doubles, whichever path runs)
    const int nb = gram_blocks(count / 2, nx, ny);
    if ((int64_t)nt * nb * kGramTile * kGramTile > kScratch) return 1;
    if (vec)
        hipLaunchKernelGGL(block_gram_kernel<true>, dim3(nb, nt), dim3(256), 0, st, a, head, n, tail, partial);
    else
        hipLaunchKernelGGL(block_gram_kernel<false>, dim3(nb, nt), dim3(256), 0, st, a, 0, n, 0, partial);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((nt * kGramTile * kGramTile + 3) / 4), dim3(256), 0, st, a, nt, nb,
                       symmetric, partial, out);
    return 0;
}

// ---- combine: out_j[e] = sum_i C[i][j] in_i[e] -------------------------------------
// acc = C[0][j] in_0[e], then acc = fma(C[i][j], in_i[e], acc) for i = 1 .. nin-1 in that
// order.  C (nin x nout, row-major, device) is read at wave-uniform addresses -- scalar
// loads into scalar registers, served by the scalar cache -- with the columns past nout
// repeating the last one (their sums are not stored).  A thread loads one (pair of)
// element(s) of every input once, kCombineAhead inputs ahead of their use, and keeps the
// NOUT sums in registers; the stores are non-temporal.
struct CombineArgs {
    const double* in[kBlockMax];
    double* out[kCombineMaxOut];
    int nin, nout;
};
constexpr int kCombineAhead = 4;

template <int NOUT, bool VEC>
__device__ __forceinline__ void combine_term(std::conditional_t<VEC, d2, double> (&acc)[NOUT],
                                             const double* __restrict__ cr, const int (&col)[NOUT],
                                             const std::conditional_t<VEC, d2, double> v) {
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        const double c = cr[col[j]];
        if constexpr (VEC) {
            acc[j].x = fma(c, v.x, acc[j].x);
            acc[j].y = fma(c, v.y, acc[j].y);
        } else {
            acc[j] = fma(c, v, acc[j]);
        }
    }
}

template <int NOUT, bool VEC>
__global__ void __launch_bounds__(256)
block_combine_kernel(const CombineArgs a, const int head, const int64_t n, const int tail,
                     const double* __restrict__ C) {
    using E = std::conditional_t<VEC, d2, double>;
    const int nin = a.nin, nout = a.nout;
    int col[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) col[j] = min(j, nout - 1);
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        E acc[NOUT];
        {
            const E v0 = __builtin_nontemporal_load((const E*)(a.in[0] + head) + i);
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j] = C[col[j]] * v0;
        }
        for (int r0 = 1; r0 < nin; r0 += kCombineAhead) {
            E v[kCombineAhead];
#pragma unroll
            for (int k = 0; k < kCombineAhead; ++k)
                if (r0 + k < nin) v[k] = __builtin_nontemporal_load((const E*)(a.in[r0 + k] + head) + i);
#pragma unroll
            for (int k = 0; k < kCombineAhead; ++k)
                if (r0 + k < nin) combine_term<NOUT, VEC>(acc, C + (r0 + k) * nout, col, v[k]);
        }
#pragma unroll
        for (int j = 0; j < NOUT; ++j)
            if (j < nout) __builtin_nontemporal_store(acc[j], (E*)(a.out[j] + head) + i);
    }
    if constexpr (VEC) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (int e = 0; e < 2; ++e) {
                if (!(e == 0 ? head : tail)) continue;
                const int64_t o = e == 0 ? 0 : head + 2 * n;
                for (int j = 0; j < nout; ++j) {
                    double acc = C[j] * a.in[0][o];
                    for (int r = 1; r < nin; ++r) acc = fma(C[r * nout + j], a.in[r][o], acc);
                    a.out[j][o] = acc;
                }
            }
        }
    }
}

template <int NOUT>
static void combine_launch_n(bool vec, int nb, hipStream_t st, const CombineArgs& a, int head, int64_t n, int tail,
                             const double* C) {
    if (vec)
        hipLaunchKernelGGL((block_combine_kernel<NOUT, true>), dim3(nb), dim3(256), 0, st, a, head, n, tail, C);
    else
        hipLaunchKernelGGL((block_combine_kernel<NOUT, false>), dim3(nb), dim3(256), 0, st, a, 0, n, 0, C);
}

int block_combine_launch(int64_t count, int nin, const double* const* ins, int nout, double* const* outs,
                         const double* coef, hipStream_t st) {
    if (nin < 1 || nin > kBlockMax || nout < 1 || nout > kCombineMaxOut || count < 1) return 1;
    CombineArgs a{};
    for (int k = 0; k < kBlockMax; ++k) a.in[k] = ins[k < nin ? k : 0];
    for (int k = 0; k < kCombineMaxOut; ++k) a.out[k] = outs[k < nout ? k : 0];
    a.nin = nin;
    a.nout = nout;
    int phase = common_phase(ins, nin, -2);
    if (phase >= 0) phase = common_phase(outs, nout, phase);
    const bool vec = phase >= 0 && count >= 4;
    const int head = vec && phase ? 1 : 0;
    const int64_t n = vec ? (count - head) / 2 : count;
    const int tail = vec ? (int)((count - head) - 2 * n) : 0;
    int64_t nb = (n + 255) / 256;
    nb = nb < 1 ? 1 : nb > 8192 ? 8192 : nb;   // (grid-stride beyond)
    if (nout == 1) combine_launch_n<1>(vec, (int)nb, st, a, head, n, tail, coef);
    else if (nout == 2) combine_launch_n<2>(vec, (int)nb, st, a, head, n, tail, coef);
    else if (nout <= 4) combine_launch_n<4>(vec, (int)nb, st, a, head, n, tail, coef);
    else if (nout <= 8) combine_launch_n<8>(vec, (int)nb, st, a, head, n, tail, coef);
    else combine_launch_n<16>(vec, (int)nb, st, a, head, n, tail, coef);
    return 0;
}

}  // namespace poms
