// Spline fields on tensor point grids (gfx950): evaluation of u_h = sum_i x_i B_i at the
// points, the load vector b_i = sum_q w_q B_i(q) f(q) and the weighted squared error
// sum_q w_q (u_h(q) - u(q))^2.  All three are Kronecker products of rectangular banded
// 1D tables (p+1 non-zero basis functions per point), applied as three 1D passes with
// lanes along the unit-stride axis 2:
//
//   evaluate / error: x --axis 0--> t0[Qc, n1, n2] --axis 1--> t1[Qc, Q1, n2] --axis 2--> out
//   load vector     : f --axis 2--> t1[Qc, Q1, n2] --axis 1--> t0[Qc, n1, n2] --axis 0--> b
//
// The large array (Qc Q1 Q2 point values) is written once (non-temporal) or read once
// (non-temporal), through LDS either way: neighbouring points share their p+1 inputs and
// neighbouring basis functions most of their points.  The intermediates are ~1/nq and
// ~1/nq^2 of it.  The error pass does not store the point values: its last pass compares,
// weights and reduces (per-thread chains, block tree, per-block partials, one reduction
// block -- deterministic).  The load vector is in gather form: one thread owns one b_i,
// no atomics.
//
// A handle owns the device tables and both intermediates, sized at creation for chunks
// of at most max_chunk_q0 axis-0 points; the run calls only launch kernels.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "launchers.hpp"     // (these two through abi_internal.hpp; named for the
#include "split_hooks.hpp"   // build's dependency scan, which reads this file only)
#include "abi_internal.hpp"
#include "poms_hip.h"

namespace poms {

namespace {

constexpr int kSeg = 1024;          // generic load pass: points of one LDS segment
constexpr int kRows = 4;            // load pass: rows of f one workgroup contracts together
constexpr int kLoadCap = 1088;      // fast load pass: most points of one tile of basis functions ((256 + 5) 4 fit)
constexpr int kLoadSlots = 5;       // fast load pass: values of a row one thread carries to LDS
constexpr int kLoadRows = 32;      // fast load pass: rows per workgroup (the coefficients stay in registers)
constexpr int kLastRows = 16;       // last expansion pass: rows of t1 staged together
constexpr int kLastCols = 288;      // ... and their columns (256 points reach at most 256 + 5 when every span has one)
constexpr int kEvalRows = 32;       // rows one workgroup of the last evaluation pass writes
constexpr int kMaxErrRows = 2048;   // bound of a thread's serial chain in the error pass
constexpr int kErrGroups = 2048;    // row groups of the error pass (partials = groups x axis-2 tiles)
constexpr int kIB = 4;              // middle contraction: basis functions per thread (they share their points)

// LDS index of element j of a row of f: one extra double per 32 breaks the nq-double lane stride
__device__ __forceinline__ int seg_pad(int j) { return j + (j >> 5); }
constexpr int kSegLds = kSeg + kSeg / 32 + 1;
constexpr int kLoadLds = kLoadCap + kLoadCap / 32 + 1;

// A pass along a middle axis k: every (o, c1, c2) is a line along k; c2 is unit-stride.
struct MidGeom {
    int64_t in_base, in_so, in_sk, in_sc1;
    int64_t out_base, out_so, out_sk, out_sc1;
    int64_t nO, nK, nC1;   // nK: output extent of the pass's axis
    int nC2;
    int k0;                // expansion: table index of output 0 (first point of the chunk)
    int kb;                // expansion: outputs per thread
    int qb, qe;            // contraction: the chunk's point range
    int accumulate;
};

__device__ __forceinline__ bool mid_line(const MidGeom& g, int64_t& in_off, int64_t& out_off) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= g.nO * g.nC1 * g.nC2) return false;
    const int64_t c2 = t % g.nC2, r = t / g.nC2;
    const int64_t c1 = r % g.nC1, o = r / g.nC1;
    in_off = g.in_base + o * g.in_so + c1 * g.in_sc1 + c2;
    out_off = g.out_base + o * g.out_so + c1 * g.out_sc1 + c2;
    return true;
}

// out[o, q, c1, c2] = sum_a B[k0 + q, a] in[o, first[k0 + q] + a, c1, c2] for the kb points q
// of blockIdx.y.  A thread keeps the p+1 inputs of its line in registers and slides the
// window as first[] advances (the points of one span share them).
template <int P>
__global__ void __launch_bounds__(256)
field_expand_mid_kernel(MidGeom g, const int* __restrict__ first, const double* __restrict__ B,
                        const double* __restrict__ in, double* __restrict__ out) {
    int64_t in_off, out_off;
    if (!mid_line(g, in_off, out_off)) return;
    const double* ip = in + in_off;
    double* op = out + out_off;
    const int qa = blockIdx.y * g.kb, qe = min(qa + g.kb, (int)g.nK);
    int cf = first[g.k0 + qa];
    double v[P + 1];
#pragma unroll
    for (int a = 0; a <= P; ++a) v[a] = ip[(int64_t)(cf + a) * g.in_sk];
    for (int q = qa; q < qe; ++q) {
        const int qt = g.k0 + q;
        const int f = first[qt];   // non-decreasing, the same in every lane
        if (f - cf > P) {
            cf = f;
#pragma unroll
            for (int a = 0; a <= P; ++a) v[a] = ip[(int64_t)(cf + a) * g.in_sk];
        } else {
            while (cf < f) {
#pragma unroll
                for (int a = 0; a < P; ++a) v[a] = v[a + 1];
                ++cf;
                v[P] = ip[(int64_t)(cf + P) * g.in_sk];
            }
        }
        const double* c = B + (int64_t)qt * (P + 1);
        double s = c[0] * v[0];
#pragma unroll
        for (int a = 1; a <= P; ++a) s = fma(c[a], v[a], s);
        op[(int64_t)q * g.out_sk] = s;
    }
}

// out[o, i, c1, c2] (+)= sum over the points q of [qlo[i], qhi[i]) n [qb, qe), ascending, of
//                         ct[(q - qlo[i]) n + i] in[o, q - qb, c1, c2]
// for the kIB basis functions i of blockIdx.y: they share most of their points, each loaded once.
__global__ void __launch_bounds__(256)
field_contract_mid_kernel(MidGeom g, const int* __restrict__ qlo, const int* __restrict__ qhi,
                          const double* __restrict__ ct, const double* __restrict__ in, double* __restrict__ out) {
    int64_t in_off, out_off;
    if (!mid_line(g, in_off, out_off)) return;
    const double* ip = in + in_off;
    double* op = out + out_off;
    const int i0 = blockIdx.y * kIB;
    int lo[kIB], a[kIB], b[kIB];
    double acc[kIB];
    int ua = g.qe, ub = g.qb;
#pragma unroll
    for (int j = 0; j < kIB; ++j) {
        const bool ok = i0 + j < g.nK;
        lo[j] = ok ? qlo[i0 + j] : 0;
        a[j] = ok ? max(lo[j], g.qb) : 0;
        b[j] = ok ? min(qhi[i0 + j], g.qe) : 0;
        if (a[j] < b[j]) { ua = min(ua, a[j]); ub = max(ub, b[j]); }
        acc[j] = 0.0;
    }
    for (int q = ua; q < ub; ++q) {
        const double v = ip[(int64_t)(q - g.qb) * g.in_sk];
#pragma unroll
        for (int j = 0; j < kIB; ++j)
            if (q >= a[j] && q < b[j]) acc[j] = fma(ct[(int64_t)(q - lo[j]) * g.nK + i0 + j], v, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < kIB; ++j)
        if (i0 + j < g.nK) {
            double* o = op + (int64_t)(i0 + j) * g.out_sk;
            *o = g.accumulate ? *o + acc[j] : acc[j];
        }
}

// Last pass of the evaluation, rows r = (q0c, q1) of t1[NR, n2]:
//   v[r, q2] = sum_a B2[q2, a] t1[r, first2[q2] + a]
// ERR = false: out[r, q2] = v (written once: non-temporal);
// ERR = true : per-block partial sums of w0 w1 w2 (v - u[r, q2])^2 (u may be null).
// A workgroup takes 256 points and rpb rows; the columns of t1 its points reach are one
// contiguous range, staged in LDS kLastRows rows at a time (read straight from t1 when a
// sparse grid spreads them over more than kLastCols).
struct LastGeom {
    int64_t NR;
    int n2, Q2, Q1;
    int rpb;      // rows per workgroup
    int q0b;
};

template <int P, bool ERR>
__global__ void __launch_bounds__(256)
field_expand_last_kernel(LastGeom g, const int* __restrict__ first2, const double* __restrict__ B2,
                         const double* __restrict__ t1, double* __restrict__ out,
                         const double* __restrict__ u, const double* __restrict__ w0,
                         const double* __restrict__ w1, const double* __restrict__ w2,
                         double* __restrict__ partial) {
    __shared__ double ts[kLastRows][kLastCols];
    __shared__ double red[4];
    const int qa = blockIdx.y * 256;
    const int q2 = qa + threadIdx.x;
    const bool active = q2 < g.Q2;
    const int qs = active ? q2 : qa;
    const int f = first2[qs];
    double c[P + 1];
#pragma unroll
    for (int a = 0; a <= P; ++a) c[a] = B2[(int64_t)qs * (P + 1) + a];
    const int fmin = first2[qa];
    const int len = first2[min(qa + 256, g.Q2) - 1] + P + 1 - fmin;   // first2 is non-decreasing
    const bool staged = len <= kLastCols;
    const int64_t r0 = (int64_t)blockIdx.x * g.rpb;
    const int64_t r1 = min(r0 + g.rpb, g.NR);
    const double wq = (ERR && active) ? w2[q2] : 0.0;
    int q0 = ERR ? g.q0b + (int)(r0 / g.Q1) : 0, q1 = ERR ? (int)(r0 % g.Q1) : 0;   // the row's points
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int64_t rb = r0; rb < r1; rb += kLastRows) {
        const int nr = (int)min((int64_t)kLastRows, r1 - rb);
        // the batch's values of u first: all in flight while t1 is staged
        double ur[ERR ? kLastRows : 1];
        if constexpr (ERR) {
#pragma unroll
            for (int r = 0; r < kLastRows; ++r)
                ur[r] = (u && active && r < nr) ? __builtin_nontemporal_load(u + (rb + r) * g.Q2 + q2) : 0.0;
        }
        if (staged) {
            // a wave stages rows wave, wave + 4, ...: their first 128 columns as one group of loads
            double tv[kLastRows / 4][2];
#pragma unroll
            for (int k = 0; k < kLastRows / 4; ++k)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int r = wave + 4 * k, j = lane + 64 * m;
                    tv[k][m] = (r < nr && j < len) ? t1[(rb + r) * g.n2 + fmin + j] : 0.0;
                }
#pragma unroll
            for (int k = 0; k < kLastRows / 4; ++k)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int r = wave + 4 * k, j = lane + 64 * m;
                    if (r < nr && j < len) ts[r][j] = tv[k][m];
                }
            if (len > 128)
                for (int r = wave; r < nr; r += 4)
                    for (int j = lane + 128; j < len; j += 64) ts[r][j] = t1[(rb + r) * g.n2 + fmin + j];
            __syncthreads();
        }
        auto point = [&](const double* tp, int r) {   // tp: the p+1 inputs of this thread's point in row rb + r
            double v = c[0] * tp[0];
#pragma unroll
            for (int a = 1; a <= P; ++a) v = fma(c[a], tp[a], v);
            if constexpr (ERR) {
                const double d = v - ur[r];
                const double w01 = w0[q0] * w1[q1];
                acc += (w01 * wq) * (d * d);
                if (++q1 == g.Q1) { q1 = 0; ++q0; }
            } else {
                __builtin_nontemporal_store(v, out + (rb + r) * g.Q2 + q2);
            }
        };
        if (staged) {
            if (active) {
#pragma unroll
                for (int r = 0; r < kLastRows; ++r)
                    if (r < nr) point(&ts[r][f - fmin], r);
            }
            __syncthreads();
        } else if (active) {
#pragma unroll
            for (int r = 0; r < kLastRows; ++r)
                if (r < nr) point(t1 + (rb + r) * g.n2 + f, r);
        }
    }
    if constexpr (ERR) {
        const double s = block_sum_256(acc, red);
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// acc[0] += sum of the partials: strided running sums of 1024 threads, the wave
// butterflies, the 16 wave sums in order.
__global__ void __launch_bounds__(1024)
field_reduce_kernel(const double* __restrict__ partial, int count, double* __restrict__ acc) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 1024) s += partial[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        acc[0] += t;
    }
}

// First pass of the load vector, rows r = (q0c, q1) of f[NR, Q2]:
//   t1[r, i2] = sum over q2 of [qlo2[i2], qhi2[i2]), ascending, of ct2[(q2 - qlo2[i2]) n2 + i2] f[r, q2]
// A workgroup takes blockDim.x basis functions, whose points are one contiguous range of
// at most kLoadCap (the host checked), and rpb rows, kRows at a time through LDS (f is
// read from HBM once).  The at most KT coefficients of a thread stay in registers.
template <int KT>
__global__ void __launch_bounds__(256)
field_contract_last_fast_kernel(int64_t NR, int n2, int Q2, int rpb, const int* __restrict__ qlo,
                                const int* __restrict__ qhi, const double* __restrict__ ct,
                                const double* __restrict__ f, double* __restrict__ t1) {
    __shared__ double fs[kRows][kLoadLds + 1];   // the last slot of a row stays 0
    const int TI = blockDim.x;
    const int i0 = blockIdx.y * TI;
    const int i2 = i0 + threadIdx.x;
    const bool active = i2 < n2;
    const int lo = active ? qlo[i2] : 0, cnt = active ? qhi[i2] - lo : 0;
    const int qmin = qlo[i0], len = qhi[min(i0 + TI, n2) - 1] - qmin;   // qlo, qhi are non-decreasing
    const bool wave_active = i0 + (int)(threadIdx.x & ~63u) < n2;
    if (threadIdx.x < kRows) fs[threadIdx.x][kLoadLds] = 0.0;
    // the thread's k-th point: its coefficient and its LDS slot (past the support: 0 times the zero slot)
    double c[KT];
    int jk[KT];
    const int off = lo - qmin;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        c[k] = k < cnt ? ct[(int64_t)k * n2 + i2] : 0.0;
        jk[k] = k < cnt ? seg_pad(off + k) : kLoadLds;
    }
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = min(r0 + rpb, NR);
    // a batch of rows goes HBM -> registers -> LDS; the next batch's loads are issued before
    // this batch is contracted, so their latency hides behind it (len <= kLoadSlots TI)
    double nx[kRows][kLoadSlots];
    auto fetch = [&](int64_t rb) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int s = 0; s < kLoadSlots; ++s) {
                const int j = threadIdx.x + s * TI;
                nx[r][s] = (j < len && rb + r < r1) ? __builtin_nontemporal_load(f + (rb + r) * Q2 + qmin + j) : 0.0;
            }
    };
    fetch(r0);
    for (int64_t rb = r0; rb < r1; rb += kRows) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int s = 0; s < kLoadSlots; ++s) {
                const int j = threadIdx.x + s * TI;
                if (j < len) fs[r][seg_pad(j)] = nx[r][s];
            }
        __syncthreads();
        if (rb + kRows < r1) fetch(rb + kRows);
        if (wave_active) {
            double acc[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) acc[r] = fma(c[k], fs[r][jk[k]], acc[r]);
            }
            if (active) {   // rows past NR land in the kRows spare rows t1 is allocated with
#pragma unroll
                for (int r = 0; r < kRows; ++r) t1[(rb + r) * n2 + i2] = acc[r];
            }
        }
        __syncthreads();
    }
}

// The same pass for any tables: 256 basis functions and kRows rows per workgroup, the
// points in LDS segments of kSeg, the coefficients read as they are used.
__global__ void __launch_bounds__(256)
field_contract_last_kernel(int64_t NR, int n2, int Q2, const int* __restrict__ qlo, const int* __restrict__ qhi,
                           const double* __restrict__ ct, const double* __restrict__ f, double* __restrict__ t1) {
    __shared__ double fs[kRows][kSegLds];
    const int i0 = blockIdx.y * 256;
    const int i2 = i0 + threadIdx.x;
    const bool active = i2 < n2;
    const int lo = active ? qlo[i2] : 0, hi = active ? qhi[i2] : 0;
    const int qmin = qlo[i0], qmax = qhi[min(i0 + 256, n2) - 1];   // qlo, qhi are non-decreasing
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    double acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = 0.0;
    for (int seg = qmin; seg < qmax; seg += kSeg) {
        const int len = min(kSeg, qmax - seg);
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const bool row_ok = r0 + r < NR;
            const double* fp = f + (r0 + r) * Q2 + seg;
            for (int j = threadIdx.x; j < len; j += 256)
                fs[r][seg_pad(j)] = row_ok ? __builtin_nontemporal_load(fp + j) : 0.0;
        }
        __syncthreads();
        const int a = max(lo, seg), b = min(hi, seg + len);
        for (int q = a; q < b; ++q) {
            const double c = ct[(int64_t)(q - lo) * n2 + i2];
            const int j = seg_pad(q - seg);
#pragma unroll
            for (int r = 0; r < kRows; ++r) acc[r] = fma(c, fs[r][j], acc[r]);
        }
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (r0 + r < NR) t1[(r0 + r) * n2 + i2] = acc[r];
    }
}

template <typename T>
int upload_vec(const std::vector<T>& h, T** dev) {
    POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dev), std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) POMS_HIP_CHECK(hipMemcpy(*dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace
}  // namespace poms

using namespace poms;

struct poms_field {
    poms_ctx* ctx = nullptr;
    int ndim = 3;
    poms_layout L{};
    int64_t s0 = 0, s1 = 0;      // plane / row strides of the padded coefficient arrays
    int n[3]{}, Q[3]{}, p[3]{};
    int max_chunk = 0;
    bool has_w = false, has_ranges = false;
    int* first[3]{};
    double* bt[3][2]{};          // (Q, p+1) values / first derivatives
    double* w[3]{};
    int *qlo[3]{}, *qhi[3]{};
    double* ct[3]{};             // (K, n) gather coefficients w B of basis function i's k-th point
    int load_kt = 0, load_ti = 0;   // fast first pass of the load vector: register bucket, tile (0: generic)
    double *t0 = nullptr, *t1 = nullptr;   // [max_chunk, n1, n2] and [max_chunk, Q1, n2]
    double* part = nullptr;
    int64_t part_n = 0;
};

namespace {

int err_rpb(int64_t NR) { return (int)std::max<int64_t>(kLastRows, (NR + kErrGroups - 1) / kErrGroups); }

template <int P>
void expand_mid_p(const MidGeom& g, dim3 grid, hipStream_t st, const int* first, const double* B, const double* in,
                  double* out) {
    hipLaunchKernelGGL(field_expand_mid_kernel<P>, grid, dim3(256), 0, st, g, first, B, in, out);
}

int expand_mid(int P, MidGeom g, hipStream_t st, const int* first, const double* B, const double* in, double* out) {
    const int64_t gx = (g.nO * g.nC1 * g.nC2 + 255) / 256;
    g.kb = 16;   // outputs per thread: fewer where the lines alone do not fill the device
    while (g.kb > 2 && gx * ((g.nK + g.kb - 1) / g.kb) < 2048) g.kb /= 2;
    const int64_t gy = (g.nK + g.kb - 1) / g.kb;
    if (gy > 65535 || gx > 0x7fffffff) { set_error("field: grid too large for one launch"); return 1; }
    const dim3 grid((unsigned)gx, (unsigned)gy);
    switch (P) {
        case 0: expand_mid_p<0>(g, grid, st, first, B, in, out); break;
        case 1: expand_mid_p<1>(g, grid, st, first, B, in, out); break;
        case 2: expand_mid_p<2>(g, grid, st, first, B, in, out); break;
        case 3: expand_mid_p<3>(g, grid, st, first, B, in, out); break;
        case 4: expand_mid_p<4>(g, grid, st, first, B, in, out); break;
        case 5: expand_mid_p<5>(g, grid, st, first, B, in, out); break;
        default: set_error("field: degree 0..5"); return 1;
    }
    return 0;
}

int contract_mid(const MidGeom& g, hipStream_t st, const int* qlo, const int* qhi, const double* ct, const double* in,
                 double* out) {
    const int64_t gx = (g.nO * g.nC1 * g.nC2 + 255) / 256, gy = (g.nK + kIB - 1) / kIB;
    if (gy > 65535 || gx > 0x7fffffff) { set_error("field: grid too large for one launch"); return 1; }
    hipLaunchKernelGGL(field_contract_mid_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, g, qlo, qhi, ct,
                       in, out);
    return 0;
}

template <int P>
void expand_last_p(bool err, const LastGeom& g, dim3 grid, hipStream_t st, const poms_field* h, const double* B2,
                   double* out, const double* u) {
    if (err)
        hipLaunchKernelGGL((field_expand_last_kernel<P, true>), grid, dim3(256), 0, st, g, h->first[2], B2, h->t1,
                           nullptr, u, h->w[0], h->w[1], h->w[2], h->part);
    else
        hipLaunchKernelGGL((field_expand_last_kernel<P, false>), grid, dim3(256), 0, st, g, h->first[2], B2, h->t1,
                           out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// the two leading expansion passes of evaluate / error: x -> t0 -> t1
int expand_lead(const poms_field* h, const double* x, const int* der, int q0b, int q0e, hipStream_t st) {
    const int Qc = q0e - q0b;
    MidGeom a{};
    a.in_base = h->L.pads[0] * h->s0 + h->L.pads[1] * h->s1 + h->L.pads[2];
    a.in_so = 0; a.in_sk = h->s0; a.in_sc1 = h->s1;
    a.out_base = 0; a.out_so = 0; a.out_sk = (int64_t)h->n[1] * h->n[2]; a.out_sc1 = h->n[2];
    a.nO = 1; a.nK = Qc; a.nC1 = h->n[1]; a.nC2 = h->n[2]; a.k0 = q0b;
    if (expand_mid(h->p[0], a, st, h->first[0], h->bt[0][der[0]], x, h->t0)) return 1;
    MidGeom b{};
    b.in_base = 0; b.in_so = (int64_t)h->n[1] * h->n[2]; b.in_sk = h->n[2]; b.in_sc1 = 0;
    b.out_base = 0; b.out_so = (int64_t)h->Q[1] * h->n[2]; b.out_sk = h->n[2]; b.out_sc1 = 0;
    b.nO = Qc; b.nK = h->Q[1]; b.nC1 = 1; b.nC2 = h->n[2]; b.k0 = 0;
    return expand_mid(h->p[1], b, st, h->first[1], h->bt[1][der[1]], h->t0, h->t1);
}

int expand_last(const poms_field* h, bool err, const int* der, int q0b, int q0e, double* out, const double* u,
                hipStream_t st, int* nblk) {
    LastGeom g{};
    g.NR = (int64_t)(q0e - q0b) * h->Q[1];
    g.n2 = h->n[2]; g.Q2 = h->Q[2]; g.Q1 = h->Q[1]; g.q0b = q0b;
    g.rpb = err ? err_rpb(g.NR) : kEvalRows;
    const int64_t gx = (g.NR + g.rpb - 1) / g.rpb, gy = (h->Q[2] + 255) / 256;
    if (gy > 65535 || gx > 0x7fffffff) { set_error("field: grid too large for one launch"); return 1; }
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (nblk) *nblk = (int)(gx * gy);
    if (err && gx * gy > h->part_n) { set_error("field: partials exceed the handle's buffer"); return 1; }
    const double* B2 = h->bt[2][der[2]];
    switch (h->p[2]) {
        case 0: expand_last_p<0>(err, g, grid, st, h, B2, out, u); break;
        case 1: expand_last_p<1>(err, g, grid, st, h, B2, out, u); break;
        case 2: expand_last_p<2>(err, g, grid, st, h, B2, out, u); break;
        case 3: expand_last_p<3>(err, g, grid, st, h, B2, out, u); break;
        case 4: expand_last_p<4>(err, g, grid, st, h, B2, out, u); break;
        case 5: expand_last_p<5>(err, g, grid, st, h, B2, out, u); break;
        default: set_error("field: degree 0..5"); return 1;
    }
    return 0;
}

template <int KT>
void contract_last_fast(const poms_field* h, int64_t NR, const double* f, hipStream_t st) {
    const dim3 grid((unsigned)((NR + kLoadRows - 1) / kLoadRows), (unsigned)((h->n[2] + h->load_ti - 1) / h->load_ti));
    hipLaunchKernelGGL(field_contract_last_fast_kernel<KT>, grid, dim3(h->load_ti), 0, st, NR, h->n[2], h->Q[2],
                       kLoadRows, h->qlo[2], h->qhi[2], h->ct[2], f, h->t1);
}

int contract_last(const poms_field* h, int64_t NR, const double* f, hipStream_t st) {
    switch (h->load_kt) {
        case 8: contract_last_fast<8>(h, NR, f, st); return 0;
        case 16: contract_last_fast<16>(h, NR, f, st); return 0;
        case 32: contract_last_fast<32>(h, NR, f, st); return 0;
        case 48: contract_last_fast<48>(h, NR, f, st); return 0;
        default: break;
    }
    const int64_t gx = (NR + kRows - 1) / kRows;
    if (gx > 0x7fffffff) { set_error("field: grid too large for one launch"); return 1; }
    const dim3 grid((unsigned)gx, (unsigned)((h->n[2] + 255) / 256));
    hipLaunchKernelGGL(field_contract_last_kernel, grid, dim3(256), 0, st, NR, h->n[2], h->Q[2], h->qlo[2], h->qhi[2],
                       h->ct[2], f, h->t1);
    return 0;
}

// Register bucket and tile of the fast first load pass, or 0 where the tables do not fit it:
// at most 48 points per basis function, at most kLoadCap points per tile of basis functions.
void pick_load_path(poms_field* h, const int* qlo, const int* qhi) {
    const int n = h->n[2];
    int K = 0;
    for (int i = 0; i < n; ++i) K = std::max(K, qhi[i] - qlo[i]);
    h->load_kt = K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : K <= 48 ? 48 : 0;
    h->load_ti = 0;
    if (!h->load_kt) return;
    for (int ti = std::min(256, ((n + 63) / 64) * 64); ti >= 64 && !h->load_ti; ti -= 64) {
        bool fits = true;
        const int cap = std::min(kLoadCap, kLoadSlots * ti);
        for (int i0 = 0; i0 < n && fits; i0 += ti) fits = qhi[std::min(i0 + ti, n) - 1] - qlo[i0] <= cap;
        if (fits) h->load_ti = ti;
    }
    if (!h->load_ti) h->load_kt = 0;
}

bool run_args_ok(const char* what, const poms_field* h, const int* der, int64_t q0b, int64_t q0e) {
    const std::string w(what);
    if (!h) { set_error(w + ": null handle"); return false; }
    if (q0b < 0 || q0e < q0b || q0e > h->Q[0]) { set_error(w + ": point range outside [0, Q0]"); return false; }
    if (q0e - q0b > h->max_chunk) { set_error(w + ": chunk exceeds max_chunk_q0"); return false; }
    if (der)
        for (int d = 0; d < 3; ++d)
            if (der[d] < 0 || der[d] > 1) { set_error(w + ": der must be 0 or 1"); return false; }
    return true;
}

}  // namespace

extern "C" {

int poms_field_destroy(poms_field* h) {
    if (!h) return 0;
    for (int d = 0; d < 3; ++d) {
        if (h->first[d]) (void)hipFree(h->first[d]);
        if (h->bt[d][0]) (void)hipFree(h->bt[d][0]);
        if (h->bt[d][1]) (void)hipFree(h->bt[d][1]);
        if (h->w[d]) (void)hipFree(h->w[d]);
        if (h->qlo[d]) (void)hipFree(h->qlo[d]);
        if (h->qhi[d]) (void)hipFree(h->qhi[d]);
        if (h->ct[d]) (void)hipFree(h->ct[d]);
    }
    if (h->t0) (void)hipFree(h->t0);
    if (h->t1) (void)hipFree(h->t1);
    if (h->part) (void)hipFree(h->part);
    delete h;
    return 0;
}

int poms_field_create(poms_ctx* ctx, int ndim, const poms_layout* layout, const int64_t* npts, const int* p,
                      const int* const* first, const double* const* basis, const double* const* weights,
                      const int* const* qlo, const int* const* qhi, int64_t max_chunk_q0, poms_field** out) {
    if (!ctx || !layout || !npts || !p || !first || !basis || !out) { set_error("poms_field_create: null argument"); return 1; }
    if (ndim < 1 || ndim > 3) { set_error("poms_field_create: ndim 1..3"); return 1; }
    for (int d = 0; d < 3; ++d) {
        if (layout->n[d] < 1 || layout->pads[d] < 0 || layout->n[d] > 0x3fffffff) { set_error("poms_field_create: bad layout"); return 1; }
        if (npts[d] < 1 || npts[d] > 0x3fffffff || p[d] < 0 || p[d] > 5 || !first[d] || !basis[d]) {
            set_error("poms_field_create: bad axis (1 <= npts, 0 <= p <= 5, tables)");
            return 1;
        }
        if (layout->n[d] < p[d] + 1) { set_error("poms_field_create: fewer basis functions than p+1"); return 1; }
        if (d < 3 - ndim && (layout->n[d] != 1 || layout->pads[d] != 0 || npts[d] != 1 || p[d] != 0)) {
            set_error("poms_field_create: unused leading axes need n = 1, pad = 0, one point, p = 0");
            return 1;
        }
    }
    const int64_t n2p = layout->n[2] + 2 * layout->pads[2];
    if (layout->pitch != 0 && layout->pitch < n2p) { set_error("poms_field_create: pitch below the padded row"); return 1; }
    if (max_chunk_q0 < 1) { set_error("poms_field_create: max_chunk_q0 >= 1"); return 1; }
    const bool has_w = weights && weights[0] && weights[1] && weights[2];
    const bool has_r = has_w && qlo && qhi && qlo[0] && qlo[1] && qlo[2] && qhi[0] && qhi[1] && qhi[2];
    // every table entry is checked here: the kernels index with them unguarded
    std::vector<double> cth[3];
    for (int d = 0; d < 3; ++d) {
        const int n = (int)layout->n[d], Q = (int)npts[d], P = p[d];
        for (int q = 0; q < Q; ++q) {
            if (first[d][q] < 0 || first[d][q] + P > n - 1) { set_error("poms_field_create: first[] outside [0, n - p - 1]"); return 1; }
            if (q && first[d][q] < first[d][q - 1]) { set_error("poms_field_create: first[] must be non-decreasing"); return 1; }
        }
        if (!has_r) continue;
        int K = 0;
        for (int i = 0; i < n; ++i) {
            const int lo = qlo[d][i], hi = qhi[d][i];
            if (lo < 0 || hi < lo || hi > Q || (i && (lo < qlo[d][i - 1] || hi < qhi[d][i - 1]))) {
                set_error("poms_field_create: qlo/qhi must be non-decreasing ranges inside [0, Q]");
                return 1;
            }
            for (int q = lo; q < hi; ++q)
                if (i < first[d][q] || i > first[d][q] + P) { set_error("poms_field_create: qlo/qhi reach outside a support"); return 1; }
            K = std::max(K, hi - lo);
        }
        if ((int64_t)K * n > (int64_t)1 << 24) { set_error("poms_field_create: support table too large"); return 1; }
        cth[d].assign((size_t)K * n, 0.0);
        for (int i = 0; i < n; ++i)
            for (int q = qlo[d][i]; q < qhi[d][i]; ++q)
                cth[d][(size_t)(q - qlo[d][i]) * n + i] =
                    weights[d][q] * basis[d][((size_t)q * (P + 1) + (i - first[d][q])) * 2];
    }
    POMS_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    poms_field* h = new poms_field;
    h->ctx = ctx;
    h->ndim = ndim;
    h->L = *layout;
    h->s1 = layout->pitch > 0 ? layout->pitch : n2p;
    h->s0 = (layout->n[1] + 2 * layout->pads[1]) * h->s1;
    h->has_w = has_w;
    h->has_ranges = has_r;
    int rc = 0;
    for (int d = 0; d < 3 && !rc; ++d) {
        const int n = (int)layout->n[d], Q = (int)npts[d], P = p[d];
        h->n[d] = n; h->Q[d] = Q; h->p[d] = P;
        std::vector<int> fi(first[d], first[d] + Q);
        std::vector<double> b0((size_t)Q * (P + 1)), b1((size_t)Q * (P + 1));
        for (size_t k = 0; k < b0.size(); ++k) { b0[k] = basis[d][2 * k]; b1[k] = basis[d][2 * k + 1]; }
        rc = upload_vec(fi, &h->first[d]) || upload_vec(b0, &h->bt[d][0]) || upload_vec(b1, &h->bt[d][1]);
        if (!rc && has_w) rc = upload_vec(std::vector<double>(weights[d], weights[d] + Q), &h->w[d]);
        if (!rc && has_r)
            rc = upload_vec(std::vector<int>(qlo[d], qlo[d] + n), &h->qlo[d]) ||
                 upload_vec(std::vector<int>(qhi[d], qhi[d] + n), &h->qhi[d]) || upload_vec(cth[d], &h->ct[d]);
    }
    if (has_r) pick_load_path(h, qlo[2], qhi[2]);
    h->max_chunk = (int)std::min<int64_t>(max_chunk_q0, h->Q[0]);
    if (!rc) {
        // t1 with kRows spare rows: the fast load pass stores whole batches of rows
        const size_t e0 = (size_t)h->max_chunk * h->n[1] * h->n[2];
        const size_t e1 = ((size_t)h->max_chunk * h->Q[1] + kRows) * h->n[2];
        const int64_t NR = (int64_t)h->max_chunk * h->Q[1];
        if (err_rpb(NR) > kMaxErrRows) { set_error("poms_field_create: chunk too large for the error reduction"); rc = 1; }
        h->part_n = (int64_t)kErrGroups * ((h->Q[2] + 255) / 256);   // err_rpb: at most kErrGroups row groups
        if (!rc && (hipMalloc(reinterpret_cast<void**>(&h->t0), e0 * sizeof(double)) != hipSuccess ||
                    hipMalloc(reinterpret_cast<void**>(&h->t1), e1 * sizeof(double)) != hipSuccess ||
                    hipMalloc(reinterpret_cast<void**>(&h->part), (size_t)h->part_n * sizeof(double)) != hipSuccess)) {
            set_error("poms_field_create: allocation failed");
            rc = 1;
        }
    }
    if (rc) { poms_field_destroy(h); return 1; }
    *out = h;
    return 0;
}

int poms_field_eval(poms_field* h, const double* x, const int* der, int64_t q0b, int64_t q0e, double* out,
                    void* stream) {
    if (!run_args_ok("poms_field_eval", h, der, q0b, q0e)) return 1;
    if (!x || !der || !out) { set_error("poms_field_eval: null argument"); return 1; }
    if (q0e == q0b) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (expand_lead(h, x, der, (int)q0b, (int)q0e, st) ||
        expand_last(h, false, der, (int)q0b, (int)q0e, out, nullptr, st, nullptr))
        return 1;
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_field_error(poms_field* h, const double* x, const int* der, const double* u, int64_t q0b, int64_t q0e,
                     double* acc, void* stream) {
    if (!run_args_ok("poms_field_error", h, der, q0b, q0e)) return 1;
    if (!x || !der || !acc) { set_error("poms_field_error: null argument"); return 1; }
    if (!h->has_w) { set_error("poms_field_error: the grid has no weights"); return 1; }
    if (q0e == q0b) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int nblk = 0;
    if (expand_lead(h, x, der, (int)q0b, (int)q0e, st) ||
        expand_last(h, true, der, (int)q0b, (int)q0e, nullptr, u, st, &nblk))
        return 1;
    hipLaunchKernelGGL(field_reduce_kernel, dim3(1), dim3(1024), 0, st, h->part, nblk, acc);
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

int poms_field_load(poms_field* h, const double* f, int64_t q0b, int64_t q0e, int accumulate, double* b,
                    void* stream) {
    if (!run_args_ok("poms_field_load", h, nullptr, q0b, q0e)) return 1;
    if (!f || !b) { set_error("poms_field_load: null argument"); return 1; }
    if (!h->has_w || !h->has_ranges) { set_error("poms_field_load: the grid has no weights or support ranges"); return 1; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int Qc = (int)(q0e - q0b);
    if (Qc > 0) {
        if (contract_last(h, (int64_t)Qc * h->Q[1], f, st)) return 1;
        MidGeom m{};
        m.in_base = 0; m.in_so = (int64_t)h->Q[1] * h->n[2]; m.in_sk = h->n[2]; m.in_sc1 = 0;
        m.out_base = 0; m.out_so = (int64_t)h->n[1] * h->n[2]; m.out_sk = h->n[2]; m.out_sc1 = 0;
        m.nO = Qc; m.nK = h->n[1]; m.nC1 = 1; m.nC2 = h->n[2]; m.qb = 0; m.qe = h->Q[1]; m.accumulate = 0;
        if (contract_mid(m, st, h->qlo[1], h->qhi[1], h->ct[1], h->t1, h->t0)) return 1;
    }
    // axis 0 into the padded vector: with an empty range (and no accumulation) zeros
    if (Qc > 0 || !accumulate) {
        MidGeom z{};
        z.in_base = 0; z.in_so = 0; z.in_sk = (int64_t)h->n[1] * h->n[2]; z.in_sc1 = h->n[2];
        z.out_base = h->L.pads[0] * h->s0 + h->L.pads[1] * h->s1 + h->L.pads[2];
        z.out_so = 0; z.out_sk = h->s0; z.out_sc1 = h->s1;
        z.nO = 1; z.nK = h->n[0]; z.nC1 = h->n[1]; z.nC2 = h->n[2];
        z.qb = (int)q0b; z.qe = (int)q0e; z.accumulate = accumulate ? 1 : 0;
        if (contract_mid(z, st, h->qlo[0], h->qhi[0], h->ct[0], h->t0, b)) return 1;
    }
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
