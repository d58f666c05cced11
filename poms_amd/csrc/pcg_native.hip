// extern "C" boundary of libpoms_hip.so (declared in include/poms_hip.h):
// poms_pcg_jacobi, the native pcg + damped-Jacobi loop with its scalar kernels and its
// opt-in speculative and graph modes.
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "abi_internal.hpp"
#include "../../include/poms_hip.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace poms;

// ---- the host-sum slots of poms_pcg_jacobi ------------------------------------
namespace poms {

// The sum of n per-block partials, added on the host in the order of
// reduce_partials_kernel (256 strided running sums, the 64-lane xor butterfly, then
// (w0 + w1) + (w2 + w3)): the same bits as the device reduction.
static double host_reduce(const double* p, int n) {
    double sv[256];
    for (int t = 0; t < 256; ++t) {
        double a = 0.0;
        for (int i = t; i < n; i += 256) a += p[i];
        sv[t] = a;
    }
    double red[4];
    for (int w = 0; w < 4; ++w) {
        double v[64], nv[64];
        for (int l = 0; l < 64; ++l) v[l] = sv[64 * w + l];
        for (int off = 32; off > 0; off >>= 1) {
            for (int l = 0; l < 64; ++l) nv[l] = v[l] + v[l ^ off];
            for (int l = 0; l < 64; ++l) v[l] = nv[l];
        }
        red[w] = v[0];
    }
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The sums `pk` (PcgSlots::pkind's bits) of a region of n blocks' partials into out:
// [dot, norm], or the three sums of EPI_JACOBI3Z; with bit 3 (EPI_RJACOBI0) a third sum
// behind [dot, norm], its partials behind the dots'.
static void reduce_region(const double* reg, int n, int pk, double* out) {
    const bool wn = pk & 1, wd = pk & 2;
    if (pk & 8) out[2] = host_reduce(reg + (size_t)2 * n, n);
    for (int i = 0; (pk & 4) && i < 3; ++i) out[i] = host_reduce(reg + (size_t)i * n, n);
    if (pk & 4) return;
    if (wn) out[wd ? 1 : 0] = host_reduce(reg, n);
    if (wd) out[0] = host_reduce(reg + (wn ? n : 0), n);
}

// poms_pcg_jacobi, one rank: ring of pinned host slots the reduction kernels
// write the host-read norms into.  seq[i] = launch sequence number that armed
// slot i (-1: never); every launch numbered below `done` is known complete (a
// value written by a later launch of the same stream has been read), so its slot
// can be re-armed without a stale write landing after the sentinel.
// ... and per slot a region of kSvPart doubles the operator launch writes its
// per-block partial sums into (no reduction launch: the host adds them in the
// reduction kernel's order when it reads the slot).  npart[i] = blocks of the
// launch that last used region i (0: none pending), pkind[i] bit 0 norm
// partials at [0, n), bit 1 dot partials after them, bit 2 three sums (EPI_JACOBI3Z),
// bit 3 (with bits 0 and 1) a third sum's partials at [2n, 3n) (EPI_RJACOBI0).
// (With a communicator only `host` is used, at fixed indices: PcgRun::hslot.)
struct PcgSlots {
    static constexpr int kSvRing = 48, kSvPart = 4096;
    // an unwritten partial in a host region: a NaN payload no reduction produces
    static constexpr uint64_t kPartUnset = 0x7ff8dead0000beefull;
    double* host = nullptr;   // kSvRing sums, pinned, device-mapped
    double* part = nullptr;   // kSvRing x kSvPart, pinned, device-mapped, armed unset
    int next = 0;
    int64_t seq_next = 0, done = 0;
    int64_t seq[kSvRing];
    int npart[kSvRing] = {}, pkind[kSvRing] = {};

    int alloc() {
        // coherent (fine-grained) and device-mapped: reduction kernels write the
        // host-read norms straight into it
        POMS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), kSvRing * sizeof(double),
                                     hipHostMallocMapped | hipHostMallocCoherent));
        POMS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&part), (size_t)kSvRing * kSvPart * sizeof(double),
                                     hipHostMallocMapped | hipHostMallocCoherent));
        part_arm(part, kSvRing * kSvPart);
        for (int64_t& q : seq) q = -1;
        return 0;
    }
    double* region(int h) { return part + (size_t)h * kSvPart; }
    // the launch just queued wrote nblk blocks' partials of the sums `pk` into slot h's region
    void pending(int h, int nblk, int pk) { npart[h] = nblk; pkind[h] = pk; }
    static int64_t host_partials_max() {   // tuning: POMS_HOST_PARTIALS (0: always reduce on the device)
        // read per launch (a getenv against a kernel launch): the parity tests switch it
        // inside one process to run the device-reduction fall-back
        const char* e = getenv("POMS_HOST_PARTIALS");
        const int64_t m = e ? std::max<int64_t>(0, atoll(e)) : kSvPart / 2;
        return std::min<int64_t>(m, kSvPart / 2);
    }
    // Arm `cnt` consecutive host slots for the next launch and return the first.
    // Direct mode takes fresh slots from a ring: a launch the loop abandoned (an
    // early damped-Jacobi stop leaves the next sweep queued) still writes ITS slot
    // later, so a slot is re-armed only once that launch is known complete -- a value
    // of a later launch has been read (launches of one stream finish in order) --
    // else the stream is drained first (advisor finding, round 2).
    int arm(int cnt, hipStream_t st) {
        if (next + cnt > kSvRing) next = 0;
        const int h = next;
        next += cnt;
        for (int i = 0; i < cnt; ++i)
            if (seq[h + i] >= done) {
                (void)hipStreamSynchronize(st);
                done = seq_next;
                break;
            }
        for (int i = 0; i < cnt; ++i) {
            reinterpret_cast<volatile double*>(host)[h + i] = -1.0;   // norms are >= 0
            seq[h + i] = seq_next;
            if (npart[h + i] > 0) {   // an abandoned launch's partials (complete by now): re-arm
                part_arm(region(h + i), pk_nsum(pkind[h + i]) * npart[h + i]);
                pending(h + i, 0, 0);
            }
        }
        ++seq_next;
        return h;
    }
    // Spin while `unset()` holds; false: the stream has drained (or failed) and it still
    // does -- never written, the launch failed.
    template <class Unset>
    static bool wait_written(Unset unset, hipStream_t st) {
        for (long k = 1; unset(); ++k) {
            __builtin_ia32_pause();
            if ((k & 4095) == 0 && hipStreamQuery(st) != hipErrorNotReady) {
                std::atomic_thread_fence(std::memory_order_seq_cst);
                if (unset()) return false;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return true;
    }
    // Wait for every partial of slot h's region and add them on the host (host_reduce)
    // into the slot's sums; 1: one was never written.
    int settle_partials(int h, hipStream_t st) {
        const int n = npart[h];
        double* reg = region(h);
        const int nsum = pk_nsum(pkind[h]);
        for (int i = 0; i < nsum * n; ++i)
            if (!wait_written([&] { return part_unset(reg + i); }, st)) return 1;
        reduce_region(reg, n, pkind[h], host + h);
        part_arm(reg, nsum * n);
        pending(h, 0, 0);
        return 0;
    }
    // Sum i of the launch that armed slot h into *out: from its region's partials where
    // it left them there, else the slot itself, spun on until the reduction kernel has
    // replaced the sentinel.  1 (message set): the launch never wrote it.
    int read(int h, int i, hipStream_t st, double* out) {
        if (npart[h] > 0) {
            if (settle_partials(h, st)) {
                set_error("poms_pcg_jacobi: a launch did not write its partial sums");
                return 1;
            }
            done = std::max(done, seq[h] + 1);
            *out = host[h + i];
            return 0;
        }
        const volatile double* v = reinterpret_cast<const volatile double*>(host) + h + i;
        if (!wait_written([&] { return *v == -1.0; }, st)) {
            set_error("poms_pcg_jacobi: a launch did not write its sum");
            return 1;
        }
        done = std::max(done, seq[h + i] + 1);   // that launch and all before it are done
        *out = *v;
        return 0;
    }
    static int pk_nsum(int pk) {   // sums of kind pk
        return (pk & 4) ? 3 : ((pk & 1) ? 1 : 0) + ((pk & 2) ? 1 : 0) + ((pk & 8) ? 1 : 0);
    }
    static bool part_unset(const double* v) { return *reinterpret_cast<const volatile uint64_t*>(v) == kPartUnset; }
    static void part_arm(double* v, int n) {
        volatile uint64_t* q = reinterpret_cast<volatile uint64_t*>(v);
        for (int i = 0; i < n; ++i) q[i] = kPartUnset;
    }
};

void pcg_slots_free(PcgSlots* s) {
    if (!s) return;
    for (double* p : {s->host, s->part})
        if (p) (void)hipHostFree(p);
    delete s;
}

}  // namespace poms

// ---- native pcg + damped-Jacobi loop (poms_pcg_jacobi) ------------------------
// The V-cycle's smoother (`sources/mg_jac.py:88,104` -> `sources/solvers.py:69-135`
// with psolve = damped_jacobi, :167-235) as one C call: the same launches, device
// scalars and stop tests as poms_amd.solvers._pcg_device, without a Python round
// trip per launch.  The host reads a norm one launch after queuing the next one
// (the GPU never waits for the host while the host waits for that norm).
namespace {

// device scalars (the sums only the host reads live in host slots / comm ring slots)
enum { SC_SR = 0, SC_PQ = 1, SC_ONE = 2, SC_ALPHA = 3, SC_ALPHA2 = 4, SC_BETA = 5, SC_SRN = 6, SC_N = 16 };
enum { H_RR0 = 0, H_RR = 1, H_J0 = 2 /* 2 slots */, H_JN = 4 /* 2 slots */ };
// a scalar folded into a flat launch: every block reads its partials, so only where
// partials x blocks stays below this (2D; not the 3D grid)
constexpr int64_t kFoldReadsMax = (int64_t)1 << 20;

// (hist: where the deferred x pass reads this iteration's alpha, PcgRun::xflush; or null)
__global__ void pcg_scalars_kernel(double* sc, int mode, double* hist) {
    if (threadIdx.x != 0) return;
    if (mode == 0) {            // alpha = s.r / p.q; pairs [1, alpha] and [alpha, beta]
        const double a = sc[SC_SR] / sc[SC_PQ];
        sc[SC_ONE] = 1.0;
        sc[SC_ALPHA] = a;
        sc[SC_ALPHA2] = a;
        if (hist != nullptr) hist[0] = a;
    } else {                    // beta = s.r / s.r_old; s.r_old <- s.r
        sc[SC_BETA] = sc[SC_SRN] / sc[SC_SR];
        sc[SC_SR] = sc[SC_SRN];
    }
}

// p.q from the apply + dot launch's per-block partials -- reduce_partials_kernel's
// order, so the same bits -- and alpha from it, in one launch (one rank: saves the
// one-block reduction launch per pcg iteration)
__global__ void __launch_bounds__(256) pcg_alpha_kernel(const double* __restrict__ part, int count, double* sc,
                                                        double* hist) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) s += part[i];
    const double pq = block_sum_256(s, red);
    if (threadIdx.x != 0) return;
    sc[SC_PQ] = pq;
    const double a = sc[SC_SR] / pq;
    sc[SC_ONE] = 1.0;
    sc[SC_ALPHA] = a;
    sc[SC_ALPHA2] = a;
    if (hist != nullptr) hist[0] = a;
}

// s.r_old <- s.r_new, where a beta folded into the x/p update left it pending and no
// folded r update follows (AlphaFold)
__global__ void pcg_sr_fix_kernel(double* sc) {
    if (threadIdx.x == 0) sc[SC_SR] = sc[SC_SRN];
}

// s.r_new from the last damped-Jacobi sweep's per-block partials (reduce_partials_kernel's
// order: the same bits), then beta = s.r_new / s.r_old and s.r_old <- s.r_new, in one
// launch (one rank: saves the one-block reduction launch per pcg iteration)
__global__ void __launch_bounds__(256) pcg_beta_kernel(const double* __restrict__ part, int count, double* sc) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) s += part[i];
    const double srn = block_sum_256(s, red);
    if (threadIdx.x != 0) return;
    sc[SC_SRN] = srn;
    sc[SC_BETA] = srn / sc[SC_SR];
    sc[SC_SR] = srn;
}

struct PcgRun {
    poms_op* op;
    poms_comm* comm;
    const poms_pcg_opts* o;
    hipStream_t st;
    void* stv;
    double* sc;
    PcgSlots& sv;
    int64_t n0 = 1;

    // The operator call of a communicator's rank.  h < 0: its sums reduced to the device
    // (nrm, dot; null: not formed); else all-reduced into host slot h as [dot, norm].
    int run_dist(int epi, const double* x, double* y, const double* b, bool wn, bool wd, double* nrm, double* dot,
                 int h) {
        const RowGeom g = row_geom(&op->L);
        int tk0 = -1;
        return poms_op_run_dist(op, comm, epi, o->omega, x, y, b, const_cast<double*>(x), g.s0, op->L.n[0],
                                (int)op->L.pads[0], op->pmax, o->prev, o->next, 1, wn ? 1 : 0, wd ? 1 : 0, nrm, dot,
                                h < 0 ? 0 : (wn ? 1 : 0) + (wd ? 1 : 0), h < 0 ? nullptr : sv.host + h,
                                h < 0 ? &tk0 : &tk[h], stv);
    }
    // one rank's launch over the whole axis 0, its partials left for the caller to reduce
    int launch(int epi, const double* x, double* y, const double* b, bool wn, bool wd, PartRoute* route = nullptr) {
        return op_run_epi(op, OpLaunch{epi, x, y, b, 0, n0, stv, o->omega, wn, wd, route});
    }
    int run(int epi, const double* x, double* y, const double* b, double* nrm, double* dot) {
        if (comm) return run_dist(epi, x, y, b, nrm, dot, nrm, dot, -1);
        return poms_op_run_reduce2(op, epi, o->omega, x, y, b, 0, n0, 0, 0, nrm, dot, 0, stv);
    }
    // alpha = s.r / p.q into the scalars (and hist_slot): p.q from the n partials at
    // `part`, or with part null from sc[SC_PQ]
    void launch_alpha(const double* part, int64_t n) {
        if (part) hipLaunchKernelGGL(pcg_alpha_kernel, dim3(1), dim3(256), 0, st, part, (int)n, sc, hist_slot);
        else hipLaunchKernelGGL(pcg_scalars_kernel, dim3(1), dim3(64), 0, st, sc, 0, hist_slot);
    }
    // beta = s.r_new / s.r_old and s.r_old <- s.r_new: s.r_new from the last sweep's
    // x . rhs partials (dot_part: reduced here), else from sc[SC_SRN]
    void launch_beta(bool from_part) {
        if (from_part) hipLaunchKernelGGL(pcg_beta_kernel, dim3(1), dim3(256), 0, st, dot_part, (int)dot_part_n, sc);
        else hipLaunchKernelGGL(pcg_scalars_kernel, dim3(1), dim3(64), 0, st, sc, 1, (double*)nullptr);
    }
    // ---- the p update formed inside the next apply + dot (EPI_PAPPLYDOT) ----
    // Where that launch runs (papply_ok), pupd only forms beta and remembers its operands;
    // the next iteration's apd_alpha launches p_next = s + beta p, q = A p_next, p_next . q
    // in one pass -- V_PUPD's fma, the apply + dot's tiles and partial slots: the same bits --
    // and p_next is never read back for the apply.  Where no apply follows, flush_pupd
    // runs the remembered update as the plain V_PUPD launch.
    const double *rem_s = nullptr, *rem_p = nullptr;
    double* rem_pn = nullptr;   // null: no p update remembered
    static bool pfold_on() {    // POMS_PCG_PFOLD=0: always the two launches (A-B; read per call: the
        const char* e = getenv("POMS_PCG_PFOLD");   // tests run both in one process)
        return !(e && e[0] == '0');
    }
    int pupd_plain(const double* s, const double* p, double* pn, const AlphaFold* bf) {
        int nb = 0;
        if (vec_flat_launch(V_PUPD, dcount, 0.0, 0.0, s + doff, p + doff, pn + doff, nullptr, nullptr, nullptr, st, &nb,
                            sc + SC_ALPHA2, bf)) {
            set_error("pcg: deferred p update not launched");
            return 1;
        }
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    int flush_pupd() {
        if (!rem_pn) return 0;
        double* pn = rem_pn;
        rem_pn = nullptr;
        return pupd_plain(rem_s, rem_p, pn, nullptr);
    }
    // q = A p, p.q and alpha: one rank folds p.q's reduction into the alpha kernel
    int apd_alpha(const double* p, double* q) {
        if (rem_pn) {   // p is the remembered p_next, not formed yet: formed by this launch
            if (p != rem_pn) { set_error("pcg: the remembered p update is not the apply's vector"); return 1; }
            OpLaunch l{EPI_PAPPLYDOT, rem_p, q, rem_s, 0, n0, stv, 0.0, false, true};
            l.y2 = rem_pn;
            l.beta_dev = sc + SC_BETA;
            if (op_run_epi(op, l)) { (void)flush_pupd(); return 1; }
            rem_pn = nullptr;
            const int64_t n = op->last_partials;
            alpha_part = op->ctx->scratch + n;
            alpha_n = n;
            return 0;
        }
        if (comm || general_form(op)) {
            if (run(EPI_APPLYDOT, p, q, p, nullptr, sc + SC_PQ) || allsum(sc + SC_PQ, 1)) return 1;
            launch_alpha(nullptr, 0);
            POMS_HIP_CHECK(hipGetLastError());
            return 0;
        }
        if (launch(EPI_APPLYDOT, p, q, p, false, true)) return 1;
        const int64_t n = op->last_partials;   // (the dot's partials at scratch + n, as poms_op_run_reduce2 reads them)
        // alpha is formed by the r update that follows (rupd: AlphaFold), or by
        // pcg_alpha_kernel when that cannot take it (flush_alpha)
        alpha_part = op->ctx->scratch + n;
        alpha_n = n;
        return 0;
    }
    const double* alpha_part = nullptr;   // p.q's partials awaiting alpha (apd_alpha)
    int64_t alpha_n = 0;
    bool sr_stale = false;                // a folded beta left s.r_old <- s.r_new pending
    int fix_sr() {
        if (!sr_stale) return 0;
        hipLaunchKernelGGL(pcg_sr_fix_kernel, dim3(1), dim3(64), 0, st, sc);
        sr_stale = false;
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    static bool fold_on() {   // POMS_ALPHA_FOLD=0: the one-block scalar kernels (tuning / A-B; read per
        const char* e = getenv("POMS_ALPHA_FOLD");   // launch: the tests run both in one process)
        return !(e && e[0] == '0');
    }
    // beta folded into the x/p update: x += alpha p, p = s + beta p with beta from the
    // last sweep's x . rhs partials (dot_part); 1 if it cannot (the caller runs
    // pcg_beta_kernel and the plain update), -1 on error
    int xpupd_beta(double* x, double* p, const double* s) {
        if (!fold_on() || !direct() || (op->L.flags & POMS_LAYOUT_GHOST_DATA) || dot_part_n < 0) return 1;
        const auto [off, count] = flat_range(row_geom(&op->L));
        if (dot_part_n * vec_flat_blocks(count, x + off) > kFoldReadsMax) return 1;
        if (fix_sr()) return -1;   // (beta reads s.r_old at sc[SC_SR])
        AlphaFold bf;
        bf.part = dot_part;
        bf.n = (int)dot_part_n;
        bf.sc = sc;
        static_assert(SC_SR == 0 && SC_BETA == 5 && SC_SRN == 6, "AlphaFold's beta slots");
        int nb = 0;
        if (vec_flat_launch(V_XPUPD, count, 0.0, 0.0, s + off, nullptr, x + off, p + off, nullptr, nullptr, st, &nb,
                            sc + SC_ALPHA2, &bf) != 0)
            return 1;
        if (hipGetLastError() != hipSuccess) { set_error("x/p update with beta: launch failed"); return -1; }
        sr_stale = true;
        return 0;
    }
    int flush_alpha() {
        if (fix_sr()) return 1;
        if (!alpha_part) return 0;
        launch_alpha(alpha_part, alpha_n);
        alpha_part = nullptr;
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // ---- deferred x updates (poms_pcg_opts.n_pbuf >= 2 on the flat path) ----
    // x is only read after the call, so x += alpha_k p_k need not run every iteration:
    // the p update writes p_{k+1} to another buffer (pupd), the terms alpha_k p_k wait in
    // `pend` with alpha_k at hist()[i], and one x pass applies them in order with the same
    // fma per term (xflush): the same bits, x read and written once per flush.
    bool defer = false;
    int64_t doff = 0, dcount = 0;      // the flat range: whole interior planes
    double* dx = nullptr;              // the call's x
    bool x_zero = false;               // x0 = None and no x pass yet: x is the zero nothing has written
    const double* pend[kXPassMax] = {};
    int npend = 0;
    double* hist_slot = nullptr;       // where the kernel that forms this iteration's alpha also stores it
    double* hist() { return sc + SC_N; }
    int push_term(const double* p) {   // alpha_k p_k, alpha_k not formed yet
        if (npend == kXPassMax && xflush(false)) return 1;
        hist_slot = hist() + npend;
        pend[npend++] = p + doff;
        return 0;
    }
    bool is_pending(const double* p) const {
        for (int j = 0; j < npend; ++j)
            if (pend[j] == p + doff) return true;
        return false;
    }
    // x = fma(alpha_j, p_j, x) over the pending terms; alt_last: the last one as the
    // early-stop branch's V_AXPBY(1, x, alpha, p) rounds it
    int xflush(bool alt_last) {
        if (npend == 0) return 0;
        XPassArgs xa;
        for (int j = 0; j < npend; ++j) xa.p[j] = pend[j];
        xa.n = npend;
        xa.from_zero = x_zero ? 1 : 0;
        xa.alt_last = alt_last ? 1 : 0;
        if (vec_xpass_launch(dcount, xa, hist(), dx + doff, st)) {
            set_error("pcg: deferred x pass not launched");
            return 1;
        }
        POMS_HIP_CHECK(hipGetLastError());
        npend = 0;
        x_zero = false;
        return 0;
    }
    // pn = s + beta p (V_XPUPD's p, x untouched): beta folded where xpupd_beta folds it,
    // else from pcg_beta_kernel / pcg_scalars_kernel as the plain x/p update takes it
    // q: where the next iteration's apply + dot writes (pupd may leave the update to that launch)
    int pupd(const double* s, const double* p, double* pn, bool part, const double* q) {
        // (n_pbuf >= 2, and a psolve buffer is never a p buffer)
        if (pn == p || pn == s || p == s) { set_error("pcg: the p update's three vectors must be distinct"); return 1; }
        if (fix_sr()) return 1;   // (beta reads s.r_old at sc[SC_SR])
        if (pfold_on() && papply_ok(op, p, s, pn, q)) {
            // beta from the one-block kernel (the launch that forms p_next reads it from
            // sc[SC_BETA]; the folded beta's bits are this kernel's)
            launch_beta(part);
            POMS_HIP_CHECK(hipGetLastError());
            rem_s = s;
            rem_p = p;
            rem_pn = pn;
            return 0;
        }
        const bool fold = part && fold_on() && dot_part_n * vec_flat_blocks(dcount, pn + doff) <= kFoldReadsMax;
        AlphaFold bf;
        if (fold) {
            bf.part = dot_part;
            bf.n = (int)dot_part_n;
            bf.sc = sc;
        } else {
            launch_beta(part);
        }
        if (pupd_plain(s, p, pn, fold ? &bf : nullptr)) return 1;
        if (fold) sr_stale = true;
        return 0;
    }
    // the last sweep of a psolve left x . rhs as per-block partials (dot_part, dot_part_n
    // blocks) for pcg_beta_kernel instead of reducing them itself (-1: it did not)
    const double* dot_part = nullptr;
    int64_t dot_part_n = -1;
    int tk[PcgSlots::kSvRing] = {};   // with a communicator: the ring ticket of host slot h
    // a sum the device needs (alpha, beta): all-reduced, the compute stream waits
    int allsum(double* d, int cnt) { return comm ? poms_allreduce_sum(comm, d, cnt, stv, 1) : 0; }
    // A value only the host reads: one rank -- the reduction kernel writes it straight
    // into the pinned (coherent, device-mapped) host slot, armed with a sentinel the
    // host spins on (~1-2 us after the kernel instead of an event wake-up, ~15 us:
    // profiles/r02/sync_probe.log); with a communicator -- a ring slot of the
    // communicator, all-reduced and copied to the host slot on the communication
    // stream while the compute stream goes on (lazy_post; the compute stream used to
    // wait for that all-reduce and copy, ~40 us per sweep in profiles/r03/proxy/).
    bool direct() const { return comm == nullptr; }
    double* hslot(int h) {
        if (direct()) return sv.host + h;
        double* d = nullptr;
        if (poms_comm_slot(comm, &d, &tk[h])) return nullptr;
        return d;
    }
    int lazy_post(int h, int cnt) { return direct() ? 0 : poms_allreduce_to_host(comm, tk[h], cnt, sv.host + h, stv); }
    // The tail of a one-rank launch of n blocks that was offered a host region for its
    // sums `pk` (PcgSlots::pkind's bits).  The partials went there (used): the region is
    // recorded for the host -- slot h's, or with h < 0 the speculative one at scur, for
    // value vi.  Else (too many blocks for the region) they are in the scratch, and
    // reductions into d are queued: [dot, norm], or the three sums.
    int sums_tail(int64_t n, int pk, bool used, int h, int vi, double* d) {
        if (used) {
            if (h >= 0) { sv.pending(h, (int)n, pk); return 0; }
            sparts.push_back(SpecPart{scur, (int)n, pk, vi});
            scur += PcgSlots::pk_nsum(pk) * n;
            return 0;
        }
        const double* scr = op->ctx->scratch;   // (norms, then dots: poms_op_run_reduce2's layout)
        const bool wn = pk & 1, wd = pk & 2;
        if ((pk & 4) ? (reduce_launch(scr, (int)n, d, st) || reduce_launch(scr + n, (int)n, d + 1, st) ||
                        reduce_launch(scr + 2 * n, (int)n, d + 2, st))
                     : ((wn && reduce_launch(scr, (int)n, d + (wd ? 1 : 0), st)) ||
                        (wd && reduce_launch(scr + n, (int)n, d, st)) ||
                        ((pk & 8) && reduce_launch(scr + 2 * n, (int)n, d + 2, st)))) {
            set_error("poms_pcg_jacobi: reduction launch failed");
            return 1;
        }
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // an operator launch whose sums only the host reads: [dot, norm] from host slot h
    int jrun(int epi, const double* x, double* y, const double* b, bool wn, bool wd, int h) {
        if (!direct()) return run_dist(epi, x, y, b, wn, wd, nullptr, nullptr, h);
        // the launch writes its partials into slot h's host region (up to
        // host_partials_max() blocks).  A/B on one box (profiles/r03/host_partials/):
        // 2D 1027^2 cycle 4.5-5.2 -> 3.6-3.7 ms, 3D 515^3 195.0-195.5 -> 194.9-195.3 ms
        PartRoute rt{sv.region(h), ((wn ? 1 : 0) + (wd ? 1 : 0)) * PcgSlots::host_partials_max()};
        if (launch(epi, x, y, b, wn, wd, &rt)) return 1;
        return sums_tail(op->last_partials, (wn ? 1 : 0) | (wd ? 2 : 0), rt.used, h, -1, sv.host + h);
    }
    // ---- the r update formed inside the first psolve launch (EPI_RJACOBI0) ----
    // Where that launch runs (rfold_ok) and the loop asks for it (poms_pcg_opts.fold_r), an
    // iteration queues no r update: its damped_jacobi starts with r_new = r - alpha q and the
    // two sweeps from zero on r_new in one pass -- V_RUPD's fma, J0's tiles and partial slots:
    // the same bits -- and r_new goes to the other of two r buffers (the launch reads r's halo
    // rows while its neighbours store theirs).  r.r comes back as a sum in tile order, fr_t,
    // which only decides (see the loop); V_RUPD's own sum is formed from the stored r_new by
    // V_SQNORM where its bits are needed.
    const double *fr_old = nullptr, *fr_q = nullptr;
    double* fr_new = nullptr;   // not null: the next damped_jacobi call starts with the fused launch
    double fr_t = 0.0;
    static bool rfold_on() {    // POMS_PCG_RFOLD=0: always the two launches (A-B; read per call: the
        const char* e = getenv("POMS_PCG_RFOLD");   // tests run both in one process)
        return !(e && e[0] == '0');
    }
    // [||x1||^2, ||dr_2||^2, ||r_new||^2 (tile order)] into slots h .. h+2
    int jrun_r(double* y, int h) {
        PartRoute rt{sv.region(h), std::min<int64_t>(3 * PcgSlots::host_partials_max(), PcgSlots::kSvPart)};
        OpLaunch l{EPI_RJACOBI0, fr_old, y, fr_q, 0, n0, stv, o->omega, true, true, &rt};
        l.y2 = fr_new;
        l.beta_dev = sc + SC_ALPHA;
        if (op_run_epi(op, l)) return 1;
        return sums_tail(op->last_partials, 1 | 2 | 8, rt.used, h, -1, sv.host + h);
    }
    // r.r of the stored r with V_RUPD's bits -> host slot h (rupd's partials and reduction)
    int sqnorm(double* r, int h) {
        int nb = 0;
        ++op->rfold_exact;
        if (vec_flat_blocks(dcount, r + doff) <= PcgSlots::host_partials_max()) {
            if (vec_flat_launch(V_SQNORM, dcount, 0.0, 0.0, nullptr, nullptr, nullptr, r + doff, nullptr, sv.region(h),
                                st, &nb)) {
                set_error("pcg: exact r.r pass not launched");
                return 1;
            }
            POMS_HIP_CHECK(hipGetLastError());
            sv.pending(h, nb, 1);
            return 0;
        }
        // (not the scratch: the last sweep's x . rhs partials wait there for beta)
        if (vec_flat_launch(V_SQNORM, dcount, 0.0, 0.0, nullptr, nullptr, nullptr, r + doff, nullptr, op->rf_part,
                            st, &nb)) {
            set_error("pcg: exact r.r pass not launched");
            return 1;
        }
        reduce_wide_launch(op->rf_part, nb, sv.host + h, st);   // (as vec_common reduces V_RUPD's partials)
        POMS_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // sweeps 1-3 from x = 0 (one rank): [||x1||^2, ||dr_2||^2, ||dr_3||^2] into slots h .. h+2
    int jrun3(const double* rhs, double* y, int h) {
        PartRoute rt{sv.region(h), 3 * PcgSlots::host_partials_max()};
        if (launch(EPI_JACOBI3Z, rhs, y, rhs, true, true, &rt)) return 1;
        return sums_tail(op->last_partials, 4, rt.used, h, -1, sv.host + h);
    }
    // `cnt` host slots for the next launch: from the ring, or with a communicator the fixed ones
    int arm(int fixed_h, int cnt) { return direct() ? sv.arm(cnt, st) : fixed_h; }
    // A failed wait (the shm sum timed out, a launch never wrote its sum) sets
    // `failed` and keeps poms_comm_wait's message: the loop returns 1 at its next
    // check instead of carrying a NaN into the stop tests (advisor, round 3).
    bool failed = false;
    double fail() { failed = true; return std::nan(""); }
    double get(int h, int i = 0) {
        if (!direct()) {
            if (poms_comm_wait(comm, tk[h])) return fail();
            return sv.host[h + i];
        }
        double v = 0.0;
        return sv.read(h, i, st, &v) ? fail() : v;
    }
    int dot(const double* a, const double* b, double* dst) {
        if (poms_vec_dot(op->ctx, &op->L, a, b, dst, stv)) return 1;
        return allsum(dst, 1);
    }
    // r -= alpha q, r.r -> host slot h.  One rank: the flat kernel writes its per-block
    // partials straight into the slot's host region (the host adds them in the order
    // of the device reduction it replaces, so the same bits) -- one launch less per
    // pcg iteration.
    // With x and p (skip_tail's last iteration): the final pass instead -- x += alpha p as
    // well, r - alpha q not kept (V_FINUPD); the same count, head, grid and per-thread
    // order, so the partials and r.r are the r update's bits.
    // norm_only (the deferred loop's last iteration under skip_tail): the sum alone
    // (V_RNORM), r and x untouched -- the x pass follows once the stop test is known.
    int rupd(double* r, const double* q, int h, double* x = nullptr, const double* p = nullptr,
             bool norm_only = false) {
        if (direct() && !(op->L.flags & POMS_LAYOUT_GHOST_DATA)) {
            const auto [off, count] = flat_range(row_geom(&op->L));
            const int64_t nbp = vec_flat_blocks(count, r + off);
            if (nbp <= PcgSlots::host_partials_max()) {
                int nb = 0;
                double* reg = sv.region(h);
                // alpha folded into this launch where its blocks' extra reads of the
                // partials are small (2D: 468 partials x ~515 blocks; not the 3D grid's
                // 495 x 65536): one launch less per pcg iteration (round 6)
                AlphaFold af;
                const bool fold = fold_on();
                if (fold && alpha_part && alpha_n * nbp <= kFoldReadsMax) {
                    af.part = alpha_part;
                    af.n = (int)alpha_n;
                    af.sc = sc;
                    af.sr = sr_stale ? SC_SRN : SC_SR;   // (a folded beta's s.r_new, copied to SC_SR by block 0)
                    af.copy_sr = sr_stale ? 1 : 0;
                    af.hist = hist_slot;
                    static_assert(SC_SR == 0 && SC_PQ == 1 && SC_ONE == 2 && SC_ALPHA == 3 && SC_ALPHA2 == 4,
                                  "AlphaFold's slots");
                } else if (flush_alpha()) {
                    return 1;
                }
                const int vop = norm_only ? V_RNORM : x ? V_FINUPD : V_RUPD;
                if (vec_flat_launch(vop, count, 0.0, 0.0, nullptr, x ? p + off : nullptr, x ? x + off : nullptr,
                                    r + off, q + off, reg, st, &nb, sc + SC_ALPHA, af.part ? &af : nullptr) == 0) {
                    if (af.part) sr_stale = false;
                    alpha_part = nullptr;
                    POMS_HIP_CHECK(hipGetLastError());
                    sv.pending(h, nb, 1);
                    return 0;
                }
            }
        }
        if (flush_alpha()) return 1;
        double* d = hslot(h);
        if (!d) return 1;
        if (norm_only) {   // (deferred: one rank, the flat kernel applies) as vec_common reduces V_RUPD's partials
            int nb = 0;
            if (vec_flat_launch(V_RNORM, dcount, 0.0, 0.0, nullptr, nullptr, nullptr, r + doff, q + doff,
                                op->ctx->scratch, st, &nb, sc + SC_ALPHA)) {
                set_error("pcg: norm-only r pass not launched");
                return 1;
            }
            reduce_wide_launch(op->ctx->scratch, nb, d, st);
            POMS_HIP_CHECK(hipGetLastError());
            return 0;
        }
        if (x ? poms_pcg_final_update_dev(op->ctx, &op->L, sc + SC_ALPHA, x, p, r, q, d, stv)
              : poms_pcg_r_update_dev(op->ctx, &op->L, sc + SC_ALPHA, r, q, d, stv))
            return 1;
        return lazy_post(h, 1);
    }
    int diag_scale_norm(const double* b, double* x, int h) {   // x = omega b / diag, ||x||^2 -> host slot h
        if (direct() && !general_form(op)) {   // partials straight into slot h's host region
            const RowGeom g = row_geom(&op->L);
            const int nb = diag_scale_blocks(op->ndim == 3, g);
            if (nb <= PcgSlots::host_partials_max()) {
                int nl = 0;
                diag_scale_launch(op->ndim == 3, op->form, g, op->pmax, (int)op->g0, o->omega, b, x, op->a0t,
                                  op->b0t, op->a1, op->b1, op->dg2a, op->dg2b, sv.region(h), st, &nl);
                POMS_HIP_CHECK(hipGetLastError());
                if (nl != nb) { set_error("diag scale: block count mismatch"); return 1; }
                op->last_partials = nb;
                sv.pending(h, nb, 1);
                return 0;
            }
        }
        if (poms_op_diag_scale(op, o->omega, b, x, 1, stv)) return 1;
        double* d = hslot(h);
        if (!d) return 1;
        reduce_launch(op->ctx->scratch, (int)op->last_partials, d, st);
        return lazy_post(h, 1);
    }

    // ---- speculative mode (spec_*): the whole smoother call is queued without reading a
    // single stop test; every host-read sum goes to its own place (a partials region of
    // op->spec_part, or op->spec_dev[i]) and the tests are evaluated once the stream has
    // drained.  If one of them fires, the call is repeated step by step (x0 restored).
    // The launches and their order are those of the step-by-step loop when no test
    // fires, so the result is the same bits (tests/test_gpu_solvers.py).
    std::vector<SpecPart> sparts;
    int64_t scur = 0;       // next free double of op->spec_part
    int sn = 0;             // next free value index
    std::vector<int> schk;  // value indices tested against jtol^2 (< fires)
    std::vector<int> srr;   // pcg r.r value index per iteration (k = 1..)
    int svals(int cnt) {
        const int i = sn;
        sn += cnt;
        return i;
    }
    // an operator launch whose sums are tested at the end: [dot, norm] at value vi
    int sjrun(int epi, const double* x, double* y, const double* b, bool wn, bool wd, int* vi_out) {
        const int cnt = (wn ? 1 : 0) + (wd ? 1 : 0);
        const int vi = svals(cnt);
        *vi_out = vi;
        double* dn = wn ? op->spec_dev + vi + (wd ? 1 : 0) : nullptr;
        double* dd = wd ? op->spec_dev + vi : nullptr;
        if (!direct()) return run(epi, x, y, b, dn, dd);
        PartRoute rt{op->spec_part + scur, poms_op::kSpecPart - scur};
        if (launch(epi, x, y, b, wn, wd, &rt)) return 1;
        return sums_tail(op->last_partials, (wn ? 1 : 0) | (wd ? 2 : 0), rt.used, -1, vi, op->spec_dev + vi);
    }
    // damped_jacobi with every sweep queued (no stop test read); as damped_jacobi below
    int spec_damped_jacobi(const double* rhs, double* A, double* B, int dot_idx, double** out) {
        const int maxit = o->jmaxiter;
        double *x = A, *xn = B;
        int fz = 0, k0;
        if (maxit >= 2 && maxit != 2 && !general_form(op)) (void)poms_op_from_zero_supported(op, &fz);
        if (fz) {   // sweeps 1, 2 from x = 0: [||x1||^2, ||dr2||^2]
            int vi;
            if (sjrun(EPI_JACOBI0, rhs, A, rhs, true, true, &vi)) return 1;
            schk.push_back(vi);
            schk.push_back(vi + 1);
            k0 = 3;
        } else {
            const int vi = svals(1);
            if (poms_op_diag_scale(op, o->omega, rhs, A, 1, stv)) return 1;
            reduce_launch(op->ctx->scratch, (int)op->last_partials, op->spec_dev + vi, st);   // (rank sums at the end)
            schk.push_back(vi);
            k0 = 2;
        }
        for (int k = k0; k <= maxit; ++k) {
            if (k == maxit) {   // the last sweep's norm cannot change the result: x . rhs instead
                if (run(EPI_JACOBI, x, xn, rhs, nullptr, sc + dot_idx) || allsum(sc + dot_idx, 1)) return 1;
            } else {
                int vi;
                if (sjrun(EPI_JACOBI, x, xn, rhs, true, false, &vi)) return 1;
                schk.push_back(vi);
            }
            std::swap(x, xn);
        }
        *out = x;
        return 0;
    }
    // damped_jacobi(A, rhs) with x0 = None into buffers {A, B} (and C: see below); the
    // last sweep also forms x . rhs into sc[dot_idx] (*dot_done = 1), else the caller
    // forms it.  Each sweep's stop test is read after the next sweep is queued -- or,
    // with a third buffer C (one rank), after the next TWO are queued: the sweeps rotate
    // over three buffers, so the two queued past a stop that fires (abandoned) cannot
    // overwrite the result, and the host's turn-around per sweep can take up to two
    // sweeps' time before the GPU waits.  The same launches and bits either way.
    int damped_jacobi(const double* rhs, double* A, double* B, int dot_idx, double** out, int* dot_done,
                      double* C = nullptr) {
        const double tol2 = o->jtol * o->jtol;
        const int maxit = o->jmaxiter;
        *dot_done = 0;
        double* bufs[3] = {A, B, C};
        const int nb = C ? 3 : 2, depth = C ? 2 : 1;
        // two sweeps per launch (one rank, 2D p = 3, three buffers; POMS_J2=0: off):
        // sweeps k, k+1 from bufs[cur] into bufs[nxt]; x_k is not stored
        static const bool j2_env = !(getenv("POMS_J2") && getenv("POMS_J2")[0] == '0');
        const bool j2 = j2_env && C && direct() && sweep2_ok(op);
        int cur = 0;                              // buffer of the latest queued x
        // an open stop test: a sweep's norm in slot h; the from-zero pair; a two-sweep
        // launch from bufs[in]; sweeps 1-3 from zero
        enum PendKind { P_SWEEP, P_ZERO2, P_PAIR, P_ZERO3, P_ZERO2R /* P_ZERO2 with the folded r update's sum */ };
        struct Pend { PendKind kind; int h, buf, in; };
        Pend q[2];
        int nq = 0, ring = 0, k0;
        int fz = 0;
        if (maxit >= 2 && maxit != 2 && !general_form(op)) (void)poms_op_from_zero_supported(op, &fz);
        // sweeps 1-3 from x = 0 in one launch where the two-sweep launches run (POMS_J2FZ=0: off)
        static const bool j3_env = !(getenv("POMS_J2FZ") && getenv("POMS_J2FZ")[0] == '0');
        if (fz && j2 && j3_env && maxit >= 4) {   // [||x1||^2, ||dr2||^2, ||dr3||^2]
            const int h0 = arm(H_J0, 3);
            if (jrun3(rhs, A, h0)) return 1;
            q[nq++] = Pend{P_ZERO3, h0, 0, -1};
            k0 = 4;
        } else if (fz && fr_new) {   // ... on rhs = fr_old - alpha fr_q, formed by the same launch
            if (rhs != fr_new) { set_error("pcg: the folded r update is not the psolve's right-hand side"); return 1; }
            const int h0 = arm(H_J0, 3);
            if (jrun_r(A, h0)) return 1;
            q[nq++] = Pend{P_ZERO2R, h0, 0, -1};
            k0 = 3;
        } else if (fz) {   // sweeps 1, 2 from x = 0 in one pass over rhs: [||x1||^2, ||dr2||^2]
            const int h0 = arm(H_J0, 2);
            if (jrun(EPI_JACOBI0, rhs, A, rhs, true, true, h0)) return 1;
            q[nq++] = Pend{P_ZERO2, h0, 0, -1};
            k0 = 3;
        } else {
            if (fr_new) { set_error("pcg: the folded r update needs the two sweeps from zero"); return 1; }
            if (maxit < 1) { set_error("pcg: jacobi maxiter < 1"); return 1; }
            const int h = arm(H_JN, 1);
            if (diag_scale_norm(rhs, A, h)) return 1;
            q[nq++] = Pend{P_SWEEP, h, 0, -1};
            ring = 1;
            k0 = 2;
        }
        // The oldest open stop test.  S_DONE: it fired, *out is the result and the call
        // returns 0; S_ERR: the call returns 1 (the values are damped_jacobi's returns).
        enum Settled { S_OPEN = -1, S_DONE = 0, S_ERR = 1 };
        auto settle = [&]() -> Settled {
            Pend f = q[0];
            q[0] = q[1];
            --nq;
            if (f.kind == P_ZERO2R) {   // r.r in tile order, read with the launch's other sums
                fr_t = get(f.h, 2);
                f.kind = P_ZERO2;
            }
            double* res = nullptr;
            // a stop before the launch's last sweep: that iterate is re-formed into the buffer
            // the next launch wrote (abandoned; queued after every sweep that reads it)
            double* xr = bufs[(f.buf + 1) % nb];
            if (f.kind == P_SWEEP) {
                if (get(f.h) < tol2) res = bufs[f.buf];
            } else if (get(f.h, 0) < tol2) {
                // after the launch's first sweep.  From zero: x1 itself, where the reference
                // stops after sweep 1.  P_PAIR: x_k, one sweep from the launch's input
                // (intact: only one launch was queued after it)
                if (f.kind == P_PAIR
                        ? launch(EPI_JACOBI, bufs[f.in], xr, rhs, false, false)
                        : poms_op_diag_scale(op, o->omega, rhs, xr, 0, stv))
                    return S_ERR;
                res = xr;
            } else if (f.kind == P_ZERO3 && get(f.h, 1) < tol2) {   // after sweep 2 of the three: x2
                if (launch(EPI_JACOBI0, rhs, xr, rhs, false, false)) return S_ERR;
                res = xr;
            } else if (get(f.h, f.kind == P_ZERO3 ? 2 : 1) < tol2) {   // after its last sweep: the launch's output
                res = bufs[f.buf];
            }
            if (failed) return S_ERR;
            if (!res) return S_OPEN;
            *out = res;
            return S_DONE;
        };
        for (int k = k0; k <= maxit; ++k) {
            const bool last = k == maxit;
            const int nxt = (cur + 1) % nb;
            int h = -1;
            if (j2 && k + 1 < maxit) {   // sweeps k, k+1: [||dr_k||^2, ||dr_{k+1}||^2]
                h = arm(H_J0, 2);
                if (jrun(EPI_JACOBI2, bufs[cur], bufs[nxt], rhs, true, true, h)) return 1;
                // every open test is read now: a two-sweep launch's own (below) after the
                // next launch, because the one after that would overwrite its input
                while (nq > 0)
                    if (const Settled s = settle(); s != S_OPEN) return s;
                q[nq++] = Pend{P_PAIR, h, nxt, cur};
                cur = nxt;
                ++k;
                continue;
            }
            if (last) {   // the last sweep's norm cannot change the result: x . rhs instead
                dot_part_n = -1;
                if (direct() && dot_idx == SC_SRN && !general_form(op)) {   // its partials wait for pcg_beta_kernel
                    if (launch(EPI_JACOBI, bufs[cur], bufs[nxt], rhs, false, true)) return 1;
                    dot_part_n = op->last_partials;
                    dot_part = op->ctx->scratch + dot_part_n;   // (where poms_op_run_reduce2 reads a dot's partials)
                } else if (run(EPI_JACOBI, bufs[cur], bufs[nxt], rhs, nullptr, sc + dot_idx) || allsum(sc + dot_idx, 1)) {
                    return 1;
                }
            } else {
                h = arm(H_JN + ring, 1);
                if (jrun(EPI_JACOBI, bufs[cur], bufs[nxt], rhs, true, false, h)) return 1;
                ring ^= 1;
            }
            cur = nxt;
            // the test of the sweep `depth` back, read after this one is queued
            if (nq == depth || (nq > 0 && (q[0].kind == P_PAIR || q[0].kind == P_ZERO3)))
                if (const Settled s = settle(); s != S_OPEN) return s;
            if (!last) q[nq++] = Pend{P_SWEEP, h, cur, -1};
        }
        while (nq > 0)   // tests still open after the last sweep (its own has none)
            if (const Settled s = settle(); s != S_OPEN) return s;
        *dot_done = k0 <= maxit ? 1 : 0;
        *out = bufs[cur];
        return 0;
    }
};

}  // namespace

// Speculative smoother call (see PcgRun::spec_*), in two halves: spec_issue queues every
// launch of the call (and, last, the copy of the device-held sums to the host); the
// values it needs later are described by R.sparts / schk / srr / sn / vrr0.
// spec_finish waits for the stream and evaluates the stop tests: 0 done, 1 error, 2 a
// stop test fired (the caller repeats the call step by step).
static int spec_issue(PcgRun& R, const double* b, double* x, int has_x0, double* const* work, int* vrr0_out) {
    poms_op* op = R.op;
    const poms_pcg_opts* o = R.o;
    poms_ctx* ctx = op->ctx;
    const poms_layout* L = &op->L;
    void* stream = R.stv;
    double *r = work[0], *q = work[1];
    double* z[3] = {work[2], work[3], work[4]};
    if (has_x0)   // x0 is kept for the step-by-step repeat
        POMS_HIP_CHECK(hipMemcpyAsync(op->spec_bak, x, padded_len(op) * sizeof(double), hipMemcpyDeviceToDevice, R.st));
    if (!has_x0) {
        if (poms_vec_fill(ctx, L, 0.0, x, stream)) return 1;
    } else if (R.run(EPI_RESID, x, r, b, nullptr, nullptr)) {
        return 1;
    }
    const int vrr0 = R.svals(1);
    *vrr0_out = vrr0;
    if (!has_x0 ? vec_copy_dot(ctx, L, b, r, op->spec_dev + vrr0, stream)   // r = b and r.r
                : poms_vec_dot(ctx, L, r, r, op->spec_dev + vrr0, stream))
        return 1;
    double* s = nullptr;
    if (R.spec_damped_jacobi(r, z[0], z[1], SC_SR, &s)) return 1;
    double* p = s;   // p keeps this buffer; the later psolves use the other two
    double* fa = nullptr;
    double* fb = nullptr;
    for (double* c : z)
        if (c != p) (fa ? fb : fa) = c;
    for (int k = 1; k <= o->maxiter; ++k) {
        if (R.run(EPI_APPLYDOT, p, q, p, nullptr, R.sc + SC_PQ) || R.allsum(R.sc + SC_PQ, 1)) return 1;
        R.launch_alpha(nullptr, 0);   // (no deferred x pass here: hist_slot is null)
        const int vrr = R.svals(1);
        R.srr.push_back(vrr);
        if (o->skip_tail && k == o->maxiter) {   // the rest of this iteration is discarded
            if (poms_pcg_final_update_dev(ctx, L, R.sc + SC_ALPHA, x, p, r, q, op->spec_dev + vrr, stream)) return 1;
            break;
        }
        if (poms_pcg_r_update_dev(ctx, L, R.sc + SC_ALPHA, r, q, op->spec_dev + vrr, stream)) return 1;
        double* sn = nullptr;
        if (R.spec_damped_jacobi(r, fa, fb, SC_SRN, &sn)) return 1;
        R.launch_beta(false);
        if (poms_pcg_xp_update_dev(ctx, L, R.sc + SC_ALPHA2, x, p, sn, stream)) return 1;
    }
    if (R.sn > poms_op::kSpecVals) { set_error("pcg speculative: too many values"); return 1; }
    if (R.comm && R.sn > 0 && poms_allreduce_sum(R.comm, op->spec_dev, R.sn, stream, 1)) return 1;
    if (R.sn > 0)
        POMS_HIP_CHECK(hipMemcpyAsync(op->spec_host, op->spec_dev, R.sn * sizeof(double), hipMemcpyDeviceToHost, R.st));
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

static int spec_finish(PcgRun& R, int vrr0, poms_pcg_info* info) {
    const poms_pcg_opts* o = R.o;
    POMS_HIP_CHECK(hipStreamSynchronize(R.st));
    std::vector<double> v(R.op->spec_host, R.op->spec_host + R.sn);
    for (const SpecPart& s : R.sparts) reduce_region(R.op->spec_part + s.off, s.n, s.kind, v.data() + s.vi);
    const double tol2 = o->jtol * o->jtol;
    for (int i : R.schk)
        if (v[i] < tol2) return 2;
    const double nrmr0 = std::sqrt(v[vrr0]);
    for (int i : R.srr)
        if (v[i] < o->tol * nrmr0) return 2;
    const double nrmr = R.srr.empty() ? nrmr0 * nrmr0 : v[R.srr.back()];
    info->niter = o->maxiter;
    info->success = 0;
    info->res_norm = std::sqrt(nrmr);
    return 0;
}

// One speculative call, through a captured graph of its launches when POMS_PCG_GRAPH
// is not 0 and there is no host-transport communicator (its callbacks synchronise).
// Graphs are cached per operator by the call's buffers, options and launch-timing
// state (kSpecGraphs entries, least recently used replaced).
static int pcg_speculative(PcgRun& R, const double* b, double* x, int has_x0, double* const* work,
                           poms_pcg_info* info) {
    poms_op* op = R.op;
    const poms_pcg_opts* o = R.o;
    // POMS_PCG_GRAPH=0: never.  Not with a communicator: the distributed operator call's
    // ring-slot and exchange bookkeeping is host-side per call (a captured RCCL
    // loopback call crashed in the attempt, r04graph logs).  A caller whose buffers
    // never repeat would capture every call: after 8 more captures than hits the
    // operator stops using graphs.
    // POMS_PCG_GRAPH=2 (opt-in, tools/graph_rccl_probe.py): graphs with a communicator
    // too -- every exchange and all-reduce of the call captured; RCCL's point-to-point
    // exchange does not survive capture, the peer transport's does (POMS_COMM_PEER=1)
    const char* ge = getenv("POMS_PCG_GRAPH");
    int host_comm = 0;
    if (R.comm && poms_comm_is_host(R.comm, &host_comm)) return 1;
    const bool comm_ok = !R.comm || (ge && ge[0] == '2' && !host_comm);
    const bool graph = !(ge && ge[0] == '0') && comm_ok && op->spec_graph_caps <= op->spec_graph_hits + 8;
    if (!graph) {
        int vrr0 = 0;
        if (spec_issue(R, b, x, has_x0, work, &vrr0)) return 1;
        return spec_finish(R, vrr0, info);
    }
    uint64_t key[16] = {};
    auto bits = [](double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; };
    key[0] = (uint64_t)(uintptr_t)b;
    key[1] = (uint64_t)(uintptr_t)x;
    for (int i = 0; i < 5; ++i) key[2 + i] = (uint64_t)(uintptr_t)work[i];
    key[7] = (uint64_t)has_x0 | ((uint64_t)(o->skip_tail ? 2 : 0)) | ((uint64_t)(uint32_t)o->maxiter << 8) | ((uint64_t)(uint32_t)o->jmaxiter << 40);
    key[8] = bits(o->tol);
    key[9] = bits(o->jtol);
    key[10] = bits(o->omega);
    key[11] = (uint64_t)(uint32_t)op->variant | ((uint64_t)(uint32_t)op->chunk << 32);
    key[12] = (uint64_t)(op->timing ? 1 : 0) | ((uint64_t)(uint32_t)op->t_epi << 8) | ((uint64_t)(uint32_t)op->t_every << 32);
    key[13] = (uint64_t)(uintptr_t)R.comm | ((uint64_t)(uint32_t)(o->prev + 1) << 48) | ((uint64_t)(uint32_t)(o->next + 1) << 56);
    {   // whatever else changes the captured launches: the setters' generation, the tile
        // geometry and ghost corners, and the env knobs read per launch (the scratch
        // layout part_off / dot_base is always op_run_split's default here)
        const char* hp = getenv("POMS_HOST_PARTIALS");
        const char* la = getenv("POMS_PCG_LOOKAHEAD");
        key[14] = op->gen ^ ((uint64_t)(uint32_t)op->tout << 20) ^ ((uint64_t)(op->ghost_corners ? 1 : 0) << 52) ^
                  ((uint64_t)(uint32_t)(hp ? atoi(hp) + 1 : 0) << 40);
        key[15] = (uint64_t)(la && la[0] ? la[0] : 0) << 56;
    }
    poms_op::SpecGraph* hit = nullptr;
    for (auto& g : op->spec_graphs)
        if (g.exec && std::memcmp(g.key, key, sizeof(key)) == 0) hit = &g;
    if (!hit) {   // capture the call's launches once
        poms_op::SpecGraph* slot = &op->spec_graphs[0];
        for (auto& g : op->spec_graphs)
            if (!g.exec || g.use < slot->use) slot = &g;
        if (slot->exec) {
            (void)hipGraphExecDestroy(slot->exec);
            slot->exec = nullptr;
        }
        // captured on a private stream (torch's default stream is the null stream, which
        // cannot be captured); nothing runs until the graph is launched on the caller's
        if (!op->cap_stream) POMS_HIP_CHECK(hipStreamCreateWithFlags(&op->cap_stream, hipStreamNonBlocking));
        const hipStream_t cst = R.st;
        void* const cstv = R.stv;
        R.st = op->cap_stream;
        R.stv = op->cap_stream;
        POMS_HIP_CHECK(hipStreamBeginCapture(R.st, hipStreamCaptureModeRelaxed));
        int vrr0 = 0;
        const int rc = spec_issue(R, b, x, has_x0, work, &vrr0);
        hipGraph_t gr = nullptr;
        const hipError_t ce = hipStreamEndCapture(R.st, &gr);
        R.st = cst;
        R.stv = cstv;
        ++op->spec_graph_caps;
        hipGraphExec_t ex = nullptr;
        hipError_t ie = hipSuccess;
        if (!rc && ce == hipSuccess) ie = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
        if (gr) (void)hipGraphDestroy(gr);
        if (rc || ce != hipSuccess || ie != hipSuccess) {
            // Nothing captured ran.  Clear the sticky error and run the call uncaptured on
            // the caller's stream (advisor, round 4: a capture or instantiate failure used
            // to fail the whole poms_pcg_jacobi call); graphs are off for this operator
            // from now on.
            (void)hipGetLastError();
            op->spec_graph_caps += 1 << 20;
            R.sparts.clear();
            R.schk.clear();
            R.srr.clear();
            R.scur = 0;
            R.sn = 0;
            int vrr0u = 0;
            if (spec_issue(R, b, x, has_x0, work, &vrr0u)) return 1;
            return spec_finish(R, vrr0u, info);
        }
        std::memcpy(slot->key, key, sizeof(key));
        slot->exec = ex;
        slot->parts = R.sparts;
        slot->chk = R.schk;
        slot->rr = R.srr;
        slot->sn = R.sn;
        slot->vrr0 = vrr0;
        hit = slot;
    } else {
        ++op->spec_graph_hits;
    }
    hit->use = ++op->spec_graph_clock;
    POMS_HIP_CHECK(hipGraphLaunch(hit->exec, R.st));
    R.sparts = hit->parts;
    R.schk = hit->chk;
    R.srr = hit->rr;
    R.sn = hit->sn;
    return spec_finish(R, hit->vrr0, info);
}

// Speculative mode is opt-in (POMS_PCG_SPEC=1): on the 2D 1024^2 cycle, measured in one
// process against the step-by-step loop, it costs 3.8 ms per cycle vs 3.1 (graph replay
// included; profiles/r04/graph): the stream drain it needs at the end of every call
// exposes the host's issue of the next phase, and the step-by-step loop's lazy reads
// already keep the queue ahead of the GPU.
static bool pcg_spec_wanted(const poms_op*, const poms_pcg_opts* o) {
    const char* e = getenv("POMS_PCG_SPEC");
    return e && e[0] == '1' && o->maxiter >= 1 && o->jmaxiter >= 3;
}

// ---- set-up: what a call needs allocated before its first launch ----
// the device scalars (then the deferred x pass's alpha_hist[kXPassMax]) and the host-sum slots
static int pcg_setup_slots(poms_op* op) {
    if (!op->sv_dev) {
        POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&op->sv_dev), (SC_N + kXPassMax) * sizeof(double)));
        POMS_HIP_CHECK(hipMemset(op->sv_dev, 0, (SC_N + kXPassMax) * sizeof(double)));
    }
    if (!op->sv) {
        PcgSlots* s = new PcgSlots;
        if (s->alloc()) { pcg_slots_free(s); return 1; }
        op->sv = s;
    }
    return 0;
}

// speculative mode's value and partials buffers, and with an x0 its backup
static int pcg_setup_spec(poms_op* op, int has_x0) {
    if (!op->spec_dev) {
        POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&op->spec_dev), poms_op::kSpecVals * sizeof(double)));
        POMS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&op->spec_host), poms_op::kSpecVals * sizeof(double),
                                     hipHostMallocDefault));
        POMS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&op->spec_part), poms_op::kSpecPart * sizeof(double),
                                     hipHostMallocMapped | hipHostMallocCoherent));
    }
    const int64_t nbak = padded_len(op);
    if (has_x0 && op->spec_bak_n < nbak) {
        if (op->spec_bak) POMS_HIP_CHECK(hipFree(op->spec_bak));
        op->spec_bak = nullptr;
        op->spec_bak_n = 0;
        POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&op->spec_bak), nbak * sizeof(double)));
        op->spec_bak_n = nbak;
    }
    return 0;
}

// The lookahead's fourth preconditioner buffer, op->la_buf.  It takes the work vectors'
// 16-B / 128-B phase (they start `shift` doubles into their allocation on the
// line-aligned layout; `like` is one of them): the flat vector kernels and v5's aligned
// tiles then run on it exactly as on the other three buffers, with the same block split
// of the sums (advisor, round 4).
static int pcg_setup_lookahead(poms_op* op, const double* like, hipStream_t st) {
    const int64_t nbuf = padded_len(op);
    const int64_t off = (int64_t)((reinterpret_cast<uintptr_t>(like) & 127) / sizeof(double));
    if (op->la_n < nbuf) {
        if (op->la_raw) POMS_HIP_CHECK(hipFree(op->la_raw));
        op->la_raw = op->la_buf = nullptr;
        op->la_n = 0;
        POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&op->la_raw), (nbuf + 16) * sizeof(double)));
        op->la_n = nbuf;
        op->la_off = -1;
    }
    if (op->la_off != off) {   // (re-)placed: zero ghosts
        POMS_HIP_CHECK(hipMemsetAsync(op->la_raw, 0, (nbuf + 16) * sizeof(double), st));
        op->la_off = off;
        op->la_buf = op->la_raw + off;
    }
    return 0;
}

// The folded r update's second r buffer, op->rf_buf: placed and zeroed as the lookahead's
// buffer above (`like` is the call's r).
static int pcg_setup_rfold(poms_op* op, const double* like, hipStream_t st) {
    const int64_t nbuf = padded_len(op);
    const int64_t off = (int64_t)((reinterpret_cast<uintptr_t>(like) & 127) / sizeof(double));
    if (op->rf_n < nbuf) {
        if (op->rf_raw) POMS_HIP_CHECK(hipFree(op->rf_raw));
        op->rf_raw = op->rf_buf = op->rf_part = nullptr;
        op->rf_n = 0;
        // (behind the vector: the exact r.r pass's partials where they do not fit a host region --
        // the scratch holds the last sweep's x . rhs partials for beta by then)
        POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&op->rf_raw), (nbuf + 16 + kScratch) * sizeof(double)));
        op->rf_part = op->rf_raw + nbuf + 16;
        op->rf_n = nbuf;
        op->rf_off = -1;
    }
    if (op->rf_off != off) {   // (re-)placed: zero ghosts
        POMS_HIP_CHECK(hipMemsetAsync(op->rf_raw, 0, (nbuf + 16) * sizeof(double), st));
        op->rf_off = off;
        op->rf_buf = op->rf_raw + off;
    }
    return 0;
}

static int pcg_jacobi_impl(poms_op* op, poms_comm* comm, const poms_pcg_opts* o, const double* b, double* x,
                           int has_x0, double* const* work, poms_pcg_info* info, void* stream) {
    if (!op || !o || !b || !x || !work || !info) { set_error("poms_pcg_jacobi: null argument"); return 1; }
    for (int i = 0; i < 5; ++i)
        if (!work[i]) { set_error("poms_pcg_jacobi: null work vector"); return 1; }
    if (o->maxiter < 0 || o->jmaxiter < 1) { set_error("poms_pcg_jacobi: bad iteration counts"); return 1; }
    POMS_HIP_CHECK(hipSetDevice(op->ctx->device));
    if (pcg_setup_slots(op)) return 1;
    const int64_t n0 = op->ndim == 3 ? op->L.n[0] : 1;
    if (pcg_spec_wanted(op, o)) {
        if (pcg_setup_spec(op, has_x0)) return 1;
        PcgRun RS{op, comm, o, as_stream(stream), stream, op->sv_dev, *op->sv, n0};
        ++op->spec_calls;
        const int rc = pcg_speculative(RS, b, x, has_x0, work, info);
        if (rc != 2) return rc;
        ++op->spec_repeats;
        // a stop test fired: the step-by-step loop from the same inputs
        if (has_x0)
            POMS_HIP_CHECK(hipMemcpyAsync(x, op->spec_bak, padded_len(op) * sizeof(double), hipMemcpyDeviceToDevice,
                                          as_stream(stream)));
    }
    PcgRun R{op, comm, o, as_stream(stream), stream, op->sv_dev, *op->sv, n0};
    poms_ctx* ctx = op->ctx;
    const poms_layout* L = &op->L;
    double *r = work[0], *q = work[1];
    double* z[3] = {work[2], work[3], work[4]};
    // Deferred x updates: p buffers passed, the flat path (one rank, no ghost data, every
    // vector on one 16-B phase); not after a speculative attempt (that mode keeps the
    // per-iteration updates, and so does its step-by-step repeat)
    const int npb = std::min<int>(o->n_pbuf, kXPassMax - 1);   // (p_1 and npb more terms fill one x pass)
    if (npb >= 2 && o->pbuf && o->maxiter >= 1 && R.direct() && !(op->L.flags & POMS_LAYOUT_GHOST_DATA) &&
        !pcg_spec_wanted(op, o)) {
        const FlatRange fr = flat_range(row_geom(&op->L));
        R.doff = fr.off;
        R.dcount = fr.count;
        R.dx = x;
        const uintptr_t ph = reinterpret_cast<uintptr_t>(x) & 15;
        bool ok = R.dcount >= 4 && (ph & 7) == 0;
        for (int i = 0; i < 5; ++i) ok = ok && (reinterpret_cast<uintptr_t>(work[i]) & 15) == ph;
        for (int i = 0; i < npb; ++i) ok = ok && o->pbuf[i] && (reinterpret_cast<uintptr_t>(o->pbuf[i]) & 15) == ph;
        R.defer = ok;
    }
    R.x_zero = R.defer && !has_x0;
    // x0 = None: x = 0 (deferred: the first x pass starts from zero instead), r = b - A.0 = b
    // exactly; else r = b - A x0
    if (!has_x0) {
        if (!R.defer && poms_vec_fill(ctx, L, 0.0, x, stream)) return 1;
    } else if (R.run(EPI_RESID, x, r, b, nullptr, nullptr)) {
        return 1;
    }
    const int hrr0 = R.arm(H_RR0, 1);
    {
        double* d = R.hslot(hrr0);
        if (!d) return 1;
        if (!has_x0 ? vec_copy_dot(ctx, L, b, r, d, stream)   // r = b and r.r in one pass
                    : poms_vec_dot(ctx, L, r, r, d, stream))
            return 1;
        if (R.lazy_post(hrr0, 1)) return 1;
    }
    const double nrmr0 = std::sqrt(R.get(hrr0));
    if (R.failed) return 1;
    // Two-sweep lookahead in the damped-Jacobi calls (one rank; POMS_PCG_LOOKAHEAD=1 /
    // 0 forces it on / off, default on for 2D operators, where the host's turn-around
    // per sweep is close to a sweep's GPU time): a fourth preconditioner buffer
    double* e4 = nullptr;
    const char* le = getenv("POMS_PCG_LOOKAHEAD");
    if (R.direct() && (le && le[0] ? le[0] == '1' : op->ndim == 2)) {
        if (pcg_setup_lookahead(op, work[2], R.st)) return 1;
        e4 = op->la_buf;
    }
    double* s = nullptr;
    int dd = 0;
    if (R.damped_jacobi(r, z[0], z[1], SC_SR, &s, &dd, e4)) return 1;
    if (!dd && R.dot(s, r, R.sc + SC_SR)) return 1;
    double* p = s;   // p keeps this buffer; later psolves use the others
    double* fp[3] = {nullptr, nullptr, nullptr};   // (fp[2]: nullptr without the lookahead)
    int nf = 0;
    for (double* c : {z[0], z[1], z[2], e4})
        if (c && c != p) fp[nf++] = c;
    int k = 0;
    int pring = 0;   // deferred: the p buffer p_{k+1} goes to
    double nrmr = nrmr0 * nrmr0;
    // The r update folded into the first psolve launch (poms_pcg_opts.fold_r; PcgRun::fr_*): the
    // deferred path under skip_tail only, where the loop's last iteration forms r.r exactly
    // (V_RNORM) whatever the iterations before it did, and where EPI_RJACOBI0 runs on these
    // vectors.  r then alternates between work[0] and op->rf_buf.
    // The stop test `r.r < tol * nrmr0` is decided from the launch's sum in tile order, t, where
    // that is safe.  Both t and V_RUPD's sum e add the same m <= dcount non-negative terms
    // fma(r_i, r_i, .), each in some order of its own, so each is within a factor 1 +- gamma_m
    // of the exact sum S of the r_i^2 (gamma_m = m u / (1 - m u), u = 2^-53: Higham, Accuracy and
    // Stability of Numerical Algorithms, 4.2; the fma rounds once per term): e >= t (1 - gamma_m)
    // / (1 + gamma_m).  So t >= tol nrmr0 (1 + g) with g >= 2 gamma_m / (1 - gamma_m) implies
    // e >= tol nrmr0: no stop, whatever e's bits.  g = 4 m u covers that with 2 m u to spare for
    // the roundings of the threshold itself (m u < 0.2: m < 2^50).  Otherwise e is formed from the
    // stored r_new by V_SQNORM -- V_RUPD's grid, order and partials: its bits -- and decides.
    bool rfold = false;
    if (R.defer && o->skip_tail && o->fold_r && PcgRun::rfold_on() && o->jmaxiter >= 3 && o->maxiter >= 2) {
        if (pcg_setup_rfold(op, r, R.st)) return 1;
        rfold = rfold_ok(op, r, q, op->rf_buf, fp[0]) && rfold_ok(op, op->rf_buf, q, r, fp[0]);
    }
    const double rf_g = 4.0 * (double)R.dcount * 0x1p-53;
    for (k = 1; k <= o->maxiter; ++k) {
        if (R.defer && R.push_term(p)) {   // (before the launch that forms alpha_k)
            (void)R.flush_pupd();          // (an error path: no apply follows a remembered p update)
            return 1;
        }
        if (R.apd_alpha(p, q)) return 1;
        if (rfold && k < o->maxiter) {
            if (R.flush_alpha()) return 1;   // (alpha at sc[SC_ALPHA], as the unfolded r update reads it there)
            double* rn = r == work[0] ? op->rf_buf : work[0];
            R.fr_old = r;
            R.fr_q = q;
            R.fr_new = rn;
            double* sn = nullptr;
            const int rc = R.damped_jacobi(rn, fp[0], fp[1], SC_SRN, &sn, &dd, fp[2]);
            R.fr_new = nullptr;
            if (rc) return 1;
            r = rn;
            if (!dd && R.dot(sn, r, R.sc + SC_SRN)) return 1;
            if (R.failed) return 1;
            const double thr = o->tol * nrmr0;
            if (!(R.fr_t >= thr * (1.0 + rf_g))) {   // inside the guard band (or not a number): V_RUPD's own sum decides
                const int hx = R.arm(H_RR, 1);
                if (R.sqnorm(r, hx)) return 1;
                nrmr = R.get(hx);
                if (R.failed) return 1;
                if (nrmr < o->tol * nrmr0) {   // the reference stops before psolve: that one is discarded
                    if (R.xflush(true)) return 1;
                    k -= 1;
                    break;
                }
            }
            double* pn = o->pbuf[pring];
            if (R.is_pending(pn) && R.xflush(false)) return 1;
            if (R.pupd(sn, p, pn, dd && R.dot_part_n >= 0, q)) return 1;   // (may leave it to the next apply + dot)
            p = pn;
            pring = (pring + 1) % npb;
            continue;
        }
        const int hrr = R.arm(H_RR, 1);
        if (R.defer && o->skip_tail && k == o->maxiter) {
            // the sum alone, then x with the rounding the stop test selects
            if (R.rupd(r, q, hrr, nullptr, nullptr, true)) return 1;
            nrmr = R.get(hrr);
            if (R.failed) return 1;
            const bool stop = nrmr < o->tol * nrmr0;
            if (R.xflush(stop)) return 1;
            if (stop) k -= 1;
            break;
        }
        if (o->skip_tail && k == o->maxiter) {
            // the reference goes on to s = psolve(A, r), s.r, beta and p (`sources/solvers.py:117-124`)
            // and returns without reading any of them: x and r.r only
            if (R.rupd(r, q, hrr, x, p)) return 1;
            nrmr = R.get(hrr);
            if (R.failed) return 1;
            if (nrmr < o->tol * nrmr0) {   // x as the early-stop branch below rounds it: the final pass left it in r
                if (poms_vec_scale(ctx, L, 1.0, r, x, stream)) return 1;
                k -= 1;
            }
            break;
        }
        if (R.rupd(r, q, hrr)) return 1;
        double* sn = nullptr;
        if (R.damped_jacobi(r, fp[0], fp[1], SC_SRN, &sn, &dd, fp[2])) return 1;   // queued before the read
        if (!dd && R.dot(sn, r, R.sc + SC_SRN)) return 1;
        nrmr = R.get(hrr);
        if (R.failed) return 1;
        if (nrmr < o->tol * nrmr0) {   // the reference stops before psolve: that one is discarded
            if (R.defer ? R.xflush(true) : poms_vec_axpby_dev(ctx, L, R.sc + SC_ONE, x, p, x, stream)) return 1;
            k -= 1;
            break;
        }
        if (R.defer) {   // p_{k+1} into the next p buffer; x first where that one still holds a pending term
            double* pn = o->pbuf[pring];
            if (R.is_pending(pn) && R.xflush(false)) return 1;
            if (R.pupd(sn, p, pn, dd && R.dot_part_n >= 0, q)) return 1;   // (may leave it to the next apply + dot)
            p = pn;
            pring = (pring + 1) % npb;
            continue;
        }
        // beta folded into the x/p update where it can be (one rank, small grids)
        const int fb = (dd && R.dot_part_n >= 0) ? R.xpupd_beta(x, p, sn) : 1;
        if (fb < 0) return 1;
        if (fb > 0) {
            if (R.fix_sr()) return 1;
            R.launch_beta(dd && R.dot_part_n >= 0);
            if (poms_pcg_xp_update_dev(ctx, L, R.sc + SC_ALPHA2, x, p, sn, stream)) return 1;
        }
    }
    // (a folded beta's pending s.r_old <- s.r_new is dropped: the next call's first
    // psolve writes s.r before anything reads it)
    R.sr_stale = false;
    if (R.flush_alpha()) return 1;
    // a p update still remembered (the loop ran out right after it): the plain launch, so
    // that the p buffers hold what they held without the fused launch
    if (R.flush_pupd()) return 1;
    // deferred: the terms still pending when the loop ran out (maxiter >= 1: from x0 = None
    // at least one x pass has run by now, x is written)
    if (R.defer && R.xflush(false)) return 1;
    if (k > o->maxiter) k = o->maxiter;
    info->niter = k;
    info->success = nrmr < o->tol * nrmr0 ? 1 : 0;
    info->res_norm = std::sqrt(nrmr);
    POMS_HIP_CHECK(hipGetLastError());
    return 0;
}

// (a peer exchange that timed out during the call fails it: poms_comm_check)
int poms_pcg_jacobi(poms_op* op, poms_comm* comm, const poms_pcg_opts* o, const double* b, double* x, int has_x0,
                    double* const* work, poms_pcg_info* info, void* stream) {
    if (pcg_jacobi_impl(op, comm, o, b, x, has_x0, work, info, stream)) return 1;
    return comm ? poms_comm_check(comm) : 0;
}
