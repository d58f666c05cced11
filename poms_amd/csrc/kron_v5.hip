// Fused Kronecker-sum operator, v5 (variant 10): the host side.  Tile geometry, the
// dispatch order of a launch's tiles (v5_sched), the events of a timed launch and the
// kron_v5_launch entry, which hands the launch to the unit that holds its build:
// kron_v5_p1.hip .. kron_v5_p5.hip (the production builds, one degree each) or
// kron_v5_diag.hip (the diagnostic builds).  The kernel, the table of production builds
// and the launch helper are in kron_v5_kernel.hpp; this file instantiates no kernel.
#include "common.hpp"
#include "kron_v5_kernel.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"   // (every header named here: the build's dependency scan reads this file only)

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace poms {

// Timing events for the next v5 launch of this thread (op_run's sampled timing):
// passed to hipExtLaunchKernel, which stamps the dispatch's own start and end.
static thread_local hipEvent_t t_v5_ev0 = nullptr, t_v5_ev1 = nullptr;
static thread_local bool t_v5_ev_used = false;

void kron_v5_set_launch_events(hipEvent_t e0, hipEvent_t e1) {
    t_v5_ev0 = e0;
    t_v5_ev1 = e1;
    t_v5_ev_used = false;
}

bool kron_v5_launch_events_used() { return t_v5_ev_used; }

// Tile geometry for the v5 kernel: halo lane-columns H on the left and output
// columns TO per tile.  Line-aligned (interior column 0 of every row on a 128-B
// line, pitch a multiple of 16): H = 8, TO = 112, so every stored row segment is
// whole lines.  Otherwise H = P rounded up to even, TO = 128 - 2H.
void kron_v5_tile(int pmax, bool aligned, int* H, int* TO) {
    if (aligned && pmax <= 8) {
        *H = 8;
        *TO = 112;
    } else {
        *H = (pmax + 1) & ~1;
        *TO = 128 - 2 * *H;
    }
}

// Dispatch order of a launch's tiles (KronGeom::sched).  The hardware hands
// workgroup b to XCD b % 8, and each XCD starts its workgroups in order, one per CU
// as CUs free up (round-robin over its 4 shader engines; r05 stamps,
// tools/v5_stamps.py --raw).  The default order gives each XCD a contiguous range
// of tiles; a range that ends on its slowest tiles -- at 515^3 the two-sweeps-from-
// zero tile rows off the axis-1 Toeplitz interior, 1.2-1.5x the others -- runs them
// in the grid's last round and stretches its tail.  This table keeps each XCD's
// range and starts its tiles in order of decreasing estimated duration (stable:
// equal tiles keep the default order, neighbours together on the XCD's L2).  The
// estimate is the tile's planes (halo included) times the measured factors of its
// slow paths.  Built once per geometry and device, outside any graph capture (a
// launch during a capture that has no table yet keeps the default order).
// POMS_V5_SCHED=0 turns it off.
static std::atomic<int> g_v5_sched{-1};

int kron_v5_set_sched(int mode) {   // poms_diag_v5_sched
    if (g_v5_sched.load() < 0) {
        const char* e = getenv("POMS_V5_SCHED");
        g_v5_sched = e ? (atoi(e) ? 1 : 0) : 1;
    }
    const int prev = g_v5_sched.load();
    if (mode >= 0) g_v5_sched = mode ? 1 : 0;
    return prev;
}

static const int* v5_sched(int P, int epi, const KronGeom& g, const ToepConst& tc, bool same12, hipStream_t st) {
    const int mode = kron_v5_set_sched(-1);
    const int nblk = g.tiles2 * g.tiles1 * g.nchunks;
    if (mode == 0 || nblk < 16) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const std::vector<int> key = {dev, P, epi, g.n0, g.n1, g.n2, g.g0, g.z_begin, g.z_end, g.z2_begin, g.z2_end,
                                  g.chunk, g.nch1, g.nchunks, g.tiles1, g.tiles2, g.tout, g.order,
                                  tc.lo0, tc.hi0, tc.lo1, tc.hi1, tc.lo2, tc.hi2};
    // a table is uploaded on the stream of the launch that built it; a launch on another
    // stream waits for the upload's event (advisor, round 5: it could otherwise read the
    // table before the copy landed) until the event is seen complete
    struct Table {
        int* d = nullptr;
        hipEvent_t ev = nullptr;
        hipStream_t st = nullptr;
        bool landed = false;
    };
    static std::mutex mu;
    static std::map<std::vector<int>, Table> cache;
    std::lock_guard<std::mutex> lk(mu);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return nullptr;
    auto it = cache.find(key);
    if (it != cache.end()) {
        Table& tb = it->second;
        if (!tb.landed) {
            // inside a capture no event may be queried or waited on (that invalidates
            // the capture): a table not yet seen landed is not used there -- the default
            // order gives the same results bitwise (the partial sums keep their slots)
            if (cs != hipStreamCaptureStatusNone) return nullptr;
            if (hipEventQuery(tb.ev) == hipSuccess) {
                tb.landed = true;
            } else {
                (void)hipGetLastError();
                if (st != tb.st && hipStreamWaitEvent(st, tb.ev, 0) != hipSuccess) {
                    (void)hipGetLastError();
                    return nullptr;
                }
            }
        }
        return tb.d;
    }
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    const int T1 = kron_v5_rows(P, epi, same12 ? 1 : 0), TO = g.tout;
    const bool j0 = epi == EPI_JACOBI0 || epi == EPI_RJACOBI0;
    std::vector<double> w(nblk);
    for (int b = 0; b < nblk; ++b) {
        const V5Tile t = v5_tile_decode(g, b);
        int z0, z1;
        chunk_planes(g, t.ch, z0, z1);
        const int r0 = t.t1 * T1, c0 = t.t2 * TO;
        double f = 1.0;
        // measured (r05 stamps, 515^3 p = 3): general axis-2 column tiles +11 % (J0) / +5 %;
        // J0 tiles that scale the ring in place +20 %, the partial last tile row +50 %
        if (!v5_toeplitz_cols(tc, c0, TO, g.n2)) f += j0 ? 0.11 : 0.05;
        if (j0 && !v5_toeplitz_rows(tc.lo1, tc.hi1, r0, T1, P)) f += 0.2;
        if (j0 && r0 + T1 > g.n1) f += 0.3;
        w[b] = (double)(z1 - z0 + 2 * P) * f;
    }
    // [0, nblk): the tile of workgroup b; [nblk, 2 nblk): that tile's slot in the
    // default order (workgroup k * 8 + x runs tile lo(x) + k)
    std::vector<int> h(2 * (size_t)nblk);
    for (int x = 0; x < 8; ++x) {
        const int lo = v5_default_tile(x, nblk), cnt = v5_xcd_tiles(x, nblk);
        std::vector<int> idx(cnt);
        for (int k = 0; k < cnt; ++k) idx[k] = lo + k;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return w[a] > w[b]; });
        for (int k = 0; k < cnt; ++k) {
            h[k * 8 + x] = idx[k];
            h[nblk + k * 8 + x] = (idx[k] - lo) * 8 + x;
        }
    }
    // stream-ordered allocation and upload on the launch's stream (no device-wide
    // synchronisation: another stream may hold a peer exchange waiting on a
    // neighbour); the host copy stays alive with the table
    static std::map<std::vector<int>, std::vector<int>> host;
    int* d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&d), h.size() * sizeof(int), st) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::vector<int>& hk = host[key];
    hk = std::move(h);
    if (hipMemcpyAsync(d, hk.data(), hk.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFreeAsync(d, st);
        host.erase(key);
        return nullptr;
    }
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, st) != hipSuccess) {
        (void)hipGetLastError();
        if (ev) (void)hipEventDestroy(ev);
        (void)hipFreeAsync(d, st);
        host.erase(key);
        return nullptr;
    }
    cache[key] = Table{d, ev, st, false};
    return d;
}

// y-store cache policy of the p <= 3 apply builds (tuning: POMS_V5_STORE = 0 nt, 1 sc1,
// 2 sc0 sc1; kV5Production)
static int store_policy() {
    static int sp = -1;
    if (sp < 0) {
        const char* e = getenv("POMS_V5_STORE");
        sp = e ? atoi(e) : 0;
        if (sp < 0 || sp > 2) sp = 0;
    }
    return sp;
}

static int v5_dispatch(int pmax, int epi, const V5Launch& a, int diag_mode) {
#ifndef POMS_V5_QUICK   // (POMS_V5_QUICK: p = 3 production builds only, for quick tuning builds)
    if (diag_mode) return kron_v5_launch_diag(diag_mode, pmax, epi, a);   // DIAGNOSTIC / tuning builds (p = 3)
#endif
    switch (pmax) {
#ifndef POMS_V5_QUICK
        case 1: return kron_v5_launch_p1(epi, store_policy(), a);
        case 2: return kron_v5_launch_p2(epi, store_policy(), a);
        case 4: return kron_v5_launch_p4(epi, store_policy(), a);   // 8-wave tiles
        case 5: return kron_v5_launch_p5(epi, store_policy(), a);
#endif
        case 3: return kron_v5_launch_p3(epi, store_policy(), a);
    }
    set_error("v5: pmax must be in 1..5");
    return 1;
}

int kron_v5_launch(int pmax, int epi, const KronPtrs& p, const KronGeom& g_in, const ToepConst& tc, int H,
                   double omega, hipStream_t st, int diag_mode) {
    const bool same12 = same_toeplitz12(tc, pmax);
    KronGeom g = g_in;
    g.sched = v5_sched(pmax, epi, g_in, tc, same12, st);
    if (H < pmax || (H & 1) || (g.tout & 1) || H + g.tout + pmax > 128) {
        set_error("v5: bad tile geometry");
        return 1;
    }
    const int rc = v5_dispatch(pmax, epi, V5Launch{p, g, tc, H, omega, st, same12, t_v5_ev0, t_v5_ev1}, diag_mode);
    if (rc == 0 && t_v5_ev0 != nullptr) {   // (every path that returns 0 has launched: the events are spent)
        t_v5_ev0 = t_v5_ev1 = nullptr;
        t_v5_ev_used = true;
    }
    return rc;
}

int kron_v5_rows(int pmax, int epi, int same12) { return v5_waves(pmax, epi, same12 != 0); }

}  // namespace poms
