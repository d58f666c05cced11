// The handle types behind include/poms_hip.h and the few internals that cross the
// files of the extern "C" boundary (abi_op.hip, which launches operators, abi_op_setup.hip,
// which makes and destroys them, abi_vec.hip, abi_transfer.hip, abi_ksolve.hip,
// pcg_native.hip; comm.hip and spline_field.hip take declarations only).
// A source that includes this header also names the three headers below itself:
// build.py's dependency scan reads a source's own quoted includes only.
#pragma once
#include "common.hpp"
#include "launchers.hpp"
#include "split_hooks.hpp"
#include "../../include/poms_hip.h"

#include <algorithm>
#include <vector>

struct poms_ctx {
    int device = 0;
    double* scratch = nullptr;  // reduction partials
};

// Host-reduced partials of one speculative launch: blocks n at offset off of the pinned
// region, kind bit 0 norm / bit 1 dot, into value index vi (+1 when both).
struct SpecPart { int64_t off; int n; int kind; int vi; };

// Where one operator launch may write its per-block partials instead of the scratch
// (OpLaunch::route, in and out): `dst` when all its sums fit in `cap` doubles, norms
// first, dots behind them; on return `used` says whether they went there.
struct PartRoute {
    double* dst = nullptr;
    int64_t cap = 0;
    bool used = false;
};

// One operator launch (op_run_epi and everything behind it): what every launch names, in
// the order a brace initialiser gives it, then what most leave at its default -- the sums
// wanted and where their partials may go, a second plane range [zb2, ze2) of axis 0 (the
// slab's other boundary), EPI_CHEBY's beta, and EPI_PAPPLYDOT's second output y2 = b + beta x
// with its beta on the device.
struct OpLaunch {
    int epi;
    const double* x;
    double* y;
    const double* b;
    int64_t zb, ze;   // planes of axis 0
    void* stream;
    double omega = 0.0;
    bool want_norm = false, want_dot = false;
    PartRoute* route = nullptr;
    int64_t zb2 = 0, ze2 = 0;
    double beta = 0.0;
    double* y2 = nullptr;
    const double* beta_dev = nullptr;
};

// poms_pcg_jacobi's host-sum slots: defined in pcg_native.hip and incomplete everywhere
// else, so no other file can touch the ring; poms_op_destroy frees them (null: nothing)
namespace poms {
struct PcgSlots;
void pcg_slots_free(PcgSlots* s);
}  // namespace poms

// Created and destroyed by abi_op_setup.hip, configured and launched by abi_op.hip.
struct poms_op {
    // ---- operator launch state (set at creation or by abi_op.hip's setters) ----
    poms_ctx* ctx = nullptr;
    int ndim = 3, form = poms::FORM_SUM, pmax = 1, chunk = 0, tout = 0;
    poms_layout L{};
    int64_t g0 = 0, n0g = 1;
    double *a0t = nullptr, *b0t = nullptr, *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr;
    double *dg2a = nullptr, *dg2b = nullptr;  // contiguous axis-2 band diagonals
    double* rdiag0 = nullptr;                  // 1/diag(A) per global plane (Toeplitz interior of axes 1, 2)
    int variant = 0;
    int last_variant = -1;    // the kernel variant the last operator launch ran (after per-call fall-backs)
    bool v2_ok = false;       // storage pads == pmax on every used axis (the Toeplitz kernels' precondition)
    bool ghost_corners = false;   // ghost edges / corners of axes 1 and 2 may be non-zero (a Cart block)
    poms::ToepConst tc{};
    double* coef = nullptr;   // FORM_STENCIL: (2p+1)^d coefficient planes of the owned rows
    int sp[3]{};              // FORM_STENCIL: stencil half-widths per axis
    // FORM_MATFREE (poms_op_create_matfree): the per-axis device tables (owned, mf_tabs),
    // the stored diagonal (dense C order, owned), the borrowed coefficient arrays at the
    // quadrature points (null: a = 1, c = mf_mass; mf_tensor: mf_a is the array of
    // component planes of a tensor coefficient) and the launch geometry
    poms::AssembleAxis mf_ax[3]{};
    std::vector<void*> mf_tabs;
    double* mf_diag = nullptr;
    const double *mf_a = nullptr, *mf_c = nullptr;
    bool mf_tensor = false;
    double mf_mass = 1.0;
    poms::MatfreeGeom mf_geom{};
    int dmask = 0;      // general forms: Dirichlet faces in the kernels' axes (poms_op_set_dirichlet)
    // general forms: the faces that carry a term (poms_op_add_face_term), in the kernels' axes.
    // FORM_STENCIL holds the terms in `coef`; FORM_MATFREE keeps each face's stencil (host sum of
    // every call, and its device copy in mf_faces, owned) and has the centres in mf_diag
    int fmask = 0;
    std::vector<double> mf_face_host[6];
    poms::MatfreeFaces mf_faces{};
    uint64_t gen = 0;  // bumped by every setter that changes the launches a graph would capture
    // op_run_split's interior launch: the communication stream's exchange and boundary
    // launch run beside it (the automatic chunking leaves them CUs, op_geom); written
    // by op_run_split only
    bool split_interior = false;

    // ---- partials layout in the scratch (written by op_run_split only, restored on return) ----
    // norms at scratch + part_off, dots at scratch + (dot_base < 0 ? nblk : dot_base) +
    // part_off: op_run_split puts two launches' partials side by side and reduces them once
    int64_t part_off = 0, dot_base = -1;
    // blocks of the last launch's partials (op_run, stencil_run, poms_op_diag_scale;
    // pcg_native.hip's diag_scale_norm writes it too)
    int64_t last_partials = 0;
    int64_t papply_launches = 0;   // EPI_PAPPLYDOT launches so far (poms_op_papply_dot_count)
    int64_t rfold_launches = 0;    // EPI_RJACOBI0 launches so far (poms_op_rjacobi0_count)
    int64_t rfold_exact = 0;       // exact r.r passes the native pcg loop queued behind them (V_SQNORM)

    // ---- native pcg loop (pcg_native.hip only; freed by poms_op_destroy) ----
    double* sv_dev = nullptr;        // device scalars, then the deferred x pass's alphas
    poms::PcgSlots* sv = nullptr;    // the pinned host-sum slots (pcg_slots_free)
    // the folded r update's second r buffer (zero ghosts), placed as la_buf is: rf_buf sits
    // rf_off doubles into rf_raw, on the work vectors' 128-B phase
    double *rf_buf = nullptr, *rf_raw = nullptr, *rf_part = nullptr;   // (rf_part: kScratch partials behind it)
    int64_t rf_off = -1, rf_n = 0;
    double* la_buf = nullptr;   // the two-sweep lookahead's fourth preconditioner buffer (zero ghosts)
    double* la_raw = nullptr;   // its allocation: la_buf sits la_off doubles in, on the work vectors' 128-B phase
    int64_t la_off = -1;
    int64_t la_n = 0;

    // ---- speculative / graph state (pcg_native.hip only; poms_op_spec_stats reads the
    // counters, poms_op_destroy frees) ----
    // poms_pcg_jacobi, speculative mode: the sweeps' per-block partials (pinned,
    // device-mapped; kSpecPart doubles), the device array of the other host-read sums,
    // and the backup of x0
    static constexpr int64_t kSpecPart = 1 << 19;
    static constexpr int kSpecVals = 4096;
    double* spec_part = nullptr;
    double* spec_dev = nullptr;
    double* spec_host = nullptr;    // kSpecVals, pinned
    double* spec_bak = nullptr;
    int64_t spec_bak_n = 0;
    struct SpecGraph {   // a captured speculative call (see pcg_speculative)
        uint64_t key[16] = {};
        hipGraphExec_t exec = nullptr;
        std::vector<SpecPart> parts;
        std::vector<int> chk, rr;
        int sn = 0, vrr0 = 0;
        int64_t use = 0;
    };
    static constexpr int kSpecGraphs = 4;
    SpecGraph spec_graphs[kSpecGraphs];
    int64_t spec_graph_clock = 0;
    int spec_graph_hits = 0, spec_graph_caps = 0;   // graphs stop when captures outnumber hits
    int spec_calls = 0, spec_repeats = 0;            // speculative calls, and those repeated step by step
    hipStream_t cap_stream = nullptr;                 // private non-blocking capture stream

    // ---- launch timing (abi_op.hip only: poms_op_timing, op_run) ----
    // HIP events around every operator launch
    struct TimedLaunch { int epi; int64_t ndof; hipEvent_t e0, e1; };
    bool timing = false;
    int t_epi = -1, t_every = 1;   // record launches of this epilogue only (-1: all), every n-th
    int64_t t_seen = 0;
    std::vector<TimedLaunch> tl;
    size_t tl_used = 0;
};

// abi_transfer.hip only
struct poms_transfer {
    poms_ctx* ctx = nullptr;
    int ndim = 3, ncm = 16;
    poms_layout L{};
    int64_t g0 = 0;
    int64_t nf[3]{}, nc[3]{};
    double* Pm[3]{};
    // banded form (coarse extent > 32): rows of P (Pb, jlo, wP) and of P^T (Rb, ilo, wR)
    bool banded = false;
    double *Pb[3]{}, *Rb[3]{};
    int *jlo[3]{}, *ilo[3]{};
    int wP[3]{}, wR[3]{};
    double *t0 = nullptr, *t1 = nullptr;
    double* part = nullptr;   // split-axis restriction partials (few lines)
    int64_t part_n = 0;
    // fused residual -> restriction: planned by poms_transfer_set_operator, which owns
    // every allocation below; poms_resid_restrict only launches
    int rform = -1;           // POMS_FORM_SUM / POMS_FORM_SINGLE; -1: no operator set
    int ncf = 0;              // columns of the fused passes' matrices (8, 12, 16, 32)
    double* Gf[6]{};          // F^T P per operator role (last axis negated), ncf columns
    double* Pf[3]{};          // P, ncf columns
    double* ru = nullptr;     // axis-0 outputs: 3 x [c0][n1][n2]
    double* rv = nullptr;     // axis-1 outputs: 3 x [c0][c1][n2]
    // the call's passes in launch order (3D: axis 0, 1, 2; 2D: axis 1, 2): geometry,
    // matrices and the ru / rv slices; x, b and the coarse output are null until a call
    // fills its copy in
    poms::MultiPass rpass[3]{};
    int nrpass = 0;
    double* mpart = nullptr;  // chunk partials of the fused passes: the largest pass's need
    int64_t mpart_n = 0;
};

// abi_ksolve.hip only
struct poms_ksolve {
    poms_ctx* ctx = nullptr;
    int ndim = 3;
    poms_layout L{};
    int64_t n0g = 1;
    int64_t ng[3]{1, 1, 1};     // global extent of every axis (the factor sizes)
    int info[3]{};
    int kl[3]{}, ku[3]{};
    std::vector<int> ipiv[3];   // absolute 0-based pivot rows (host copy, for callers)
    double *Ld[3]{}, *Ud[3]{};
    int* pivd[3]{};
    poms::BandLU f[3]{};
};

// the operator forms that run the general kernels (their own partials layout, no
// two-sweeps-from-zero, a stored diagonal): the stored stencil and the matrix-free form
inline bool general_form(const poms_op* o) { return o->form == poms::FORM_STENCIL || o->form == poms::FORM_MATFREE; }

// a slab of axis 0 or a Cart block: some neighbour's rows act through exchanged ghosts
inline bool distributed(const poms_op* o) {
    return o->g0 != 0 || (o->ndim == 3 && o->L.n[0] != o->n0g) || (o->L.flags & POMS_LAYOUT_GHOST_DATA);
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool layout_ok(const poms_layout* L) {
    if (!L) return false;
    for (int d = 0; d < 3; ++d)
        if (L->n[d] < 1 || L->pads[d] < 0) return false;
    return L->pitch == 0 || L->pitch >= L->n[2] + 2 * L->pads[2];
}

inline poms::RowGeom row_geom(const poms_layout* L) {
    poms::RowGeom g;
    const int64_t c2 = L->pitch > 0 ? L->pitch : L->n[2] + 2 * L->pads[2];
    const int64_t c1 = L->n[1] + 2 * L->pads[1];
    g.s1 = c2;
    g.s0 = c1 * c2;
    g.n0 = (int)L->n[0];
    g.n1 = (int)L->n[1];
    g.n2 = (int)L->n[2];
    g.pd0 = (int)L->pads[0];
    g.pd1 = (int)L->pads[1];
    g.pd2 = (int)L->pads[2];
    return g;
}

// the general-stencil kernels' geometry: half-widths sp[3], planes [zb, ze) + [zb2, ze2)
inline poms::StencilGeom stencil_geom(const poms::RowGeom& r, const int* sp, int64_t zb, int64_t ze, int64_t zb2,
                                      int64_t ze2, int dmask) {
    return {r.s0, r.s1, r.n0, r.n1, r.n2, r.pd0, r.pd1, r.pd2, sp[0], sp[1], sp[2],
            2 * sp[0] + 1, 2 * sp[1] + 1, 2 * sp[2] + 1, (int64_t)r.n0 * r.n1 * r.n2,
            (int)zb, (int)ze, (int)zb2, (int)ze2, dmask};
}

// doubles of one of the operator's vectors, ghost planes included
inline int64_t padded_len(const poms_op* o) { return (int64_t)(o->L.n[0] + 2 * o->L.pads[0]) * row_geom(&o->L).s0; }

inline int upload(const double* host, size_t n, double** dev) {
    POMS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(dev), std::max<size_t>(n, 1) * sizeof(double)));
    if (n) POMS_HIP_CHECK(hipMemcpy(*dev, host, n * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

namespace poms {

// abi_op.hip
bool error_is_set();                         // a message is waiting in poms_last_error
int ctx_device(const poms_ctx* ctx);         // for the sources that see poms_ctx opaque
bool sweep2_ok(const poms_op* o);
// EPI_PAPPLYDOT can run y2 = b + beta x, y = A y2 on these vectors with the bits of the flat
// p update followed by EPI_APPLYDOT on y2 (papply_ok's comment in abi_op.hip)
bool papply_ok(const poms_op* o, const double* x, const double* b, const double* y2, const double* y);
// EPI_RJACOBI0 can run y2 = x - alpha b and the two sweeps from zero on y2 with the bits of the
// flat r update followed by EPI_JACOBI0 (rfold_ok's comment in abi_op.hip)
bool rfold_ok(const poms_op* o, const double* x, const double* b, const double* y2, const double* y);
int op_run_epi(poms_op* op, const OpLaunch& q);
int op_run_split(poms_op* op, const OpLaunch& interior, int64_t b1s, int64_t b1e, int64_t b2s, int64_t b2e,
                 double* norm_out, double* dot_out, const SplitHooks& h);

// abi_vec.hip
int vec_copy_dot(poms_ctx* ctx, const poms_layout* L, const double* x, double* z, double* out_dev,
                 void* stream);

}  // namespace poms
