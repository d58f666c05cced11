// The diagnostic / tuning builds of kron_v5_kernel (p = 3; variants 101-114 of the
// variant table) and the MODE 6 stamp buffer with its read-out.  Not on any production
// path: kron_v5_launch (kron_v5.hip) comes here only with a diagnostic mode set.
#define POMS_V5_STAMP_UNIT   // g_v5_stamps is defined in this unit (kron_v5_kernel.hpp)
#include "common.hpp"
#include "kron_v5_kernel.hpp"
#include "launchers.hpp"
#include "wave_ops.hpp"   // (every header named here: the build's dependency scan reads this file only)

#include <vector>

namespace poms {

#ifndef POMS_V5_QUICK   // (POMS_V5_QUICK: p = 3 production builds only, for quick tuning builds)

// Modes 3-9: the cache policies one by one, on the apply (4 x planes), the residual and
// the Jacobi sweep (3 x planes, the 2-deep b ring).
struct V5DiagPolicy {
    int cp;
    bool xh;   // Jacobi x_in from the register history
};
constexpr V5DiagPolicy kV5DiagPolicy[] = {
    /* 3 */ {CP_Y_NT, false},
    /* 4 */ {CP_Y_NT | CP_B_NT, false},
    /* 5 */ {CP_Y_NT | CP_B_NT | CP_X_NT, false},
    /* 6 */ {CP_Y_NT, true},
    /* 7 */ {0, false},                                  // default policy everywhere
    /* 8 */ {CP_B_NT, false},
    /* 9 */ {CP_Y_NT | CP_B_NT | CP_OWN_NT, true},       // + nt on the rows no other tile reads
};
static_assert(sizeof(kV5DiagPolicy) / sizeof(kV5DiagPolicy[0]) == 7, "modes 3-9");

// A policy that spells out the production build (mode 4 on the apply) is launched from
// the production unit: a kernel is compiled in one unit only.
template <int EPI, int D, int CP, bool XH>
static int v5_launch_tuning(const V5Launch& a) {
    constexpr int R = v5_production(3, EPI);
    if constexpr (R >= 0 && kV5Production[R].D == D && kV5Production[R].cp == CP && kV5Production[R].xh == XH)
        return kron_v5_launch_p3(EPI, 0, a);
    else
        return v5_launch<3, EPI, D, 0, CP, XH>(a);
}

template <int MODE>   // diagnostic mode MODE: row MODE - 3 of kV5DiagPolicy
static int v5_launch_policy(int epi, const V5Launch& a) {
    constexpr V5DiagPolicy d = kV5DiagPolicy[MODE - 3];
    switch (epi) {
        case EPI_APPLY: return v5_launch_tuning<EPI_APPLY, 4, d.cp, d.xh>(a);
        case EPI_RESID: return v5_launch_tuning<EPI_RESID, 3, d.cp, d.xh>(a);
        case EPI_JACOBI: return v5_launch_tuning<EPI_JACOBI, 3, d.cp, d.xh>(a);
    }
    set_error("v5 diag mode: bad mode / epilogue");
    return 1;
}

int kron_v5_launch_diag(int diag_mode, int pmax, int epi, const V5Launch& a) {
    if (pmax != 3) { set_error("v5 diag mode: p = 3 only"); return 1; }
    // the production builds these modes start from
    constexpr int APPLY = v5_production(3, EPI_APPLY), JACOBI = v5_production(3, EPI_JACOBI),
                  JACOBI0 = v5_production(3, EPI_JACOBI0);
    if (diag_mode == 13) {   // Jacobi sweep (production ring depths) + nt on the x rows no other tile reads
        if (epi != EPI_JACOBI) { set_error("v5 diag mode 13: Jacobi only"); return 1; }
        return v5_launch_row<3, JACOBI, 0, CP_OWN_NT>(a);
    }
    if (diag_mode >= 10 && diag_mode <= 12) {   // two sweeps from zero: 10 no sums, 11 no x1 scaling, 12 both
        if (epi != EPI_JACOBI0) { set_error("v5 diag mode 10-12: two sweeps from zero only"); return 1; }
        return diag_mode == 10 ? v5_launch_row<3, JACOBI0, 3>(a)
             : diag_mode == 11 ? v5_launch_row<3, JACOBI0, 4>(a)
                               : v5_launch_row<3, JACOBI0, 5>(a);
    }
    if (diag_mode == 14) {   // stamped march (MODE 6): the apply's, the Jacobi sweep's or J0's production build
        if (epi == EPI_APPLY) return v5_launch_row<3, APPLY, 6>(a);
        if (epi == EPI_JACOBI) return v5_launch_row<3, JACOBI, 6>(a);
        if (epi == EPI_JACOBI0) return v5_launch_row<3, JACOBI0, 6>(a);
        set_error("v5 diag mode 14: apply / Jacobi / two sweeps from zero only");
        return 1;
    }
    if (diag_mode <= 2) {   // 1 = memory only (the apply's cache policy), 2 = arithmetic only (apply)
        if (epi != EPI_APPLY) { set_error("v5 diag mode 1/2: apply only"); return 1; }
        return diag_mode == 1 ? v5_launch_row<3, APPLY, 1>(a) : v5_launch<3, EPI_APPLY, 4, 2>(a);
    }
    switch (diag_mode) {
        case 3: return v5_launch_policy<3>(epi, a);
        case 4: return v5_launch_policy<4>(epi, a);
        case 5: return v5_launch_policy<5>(epi, a);
        case 6: return v5_launch_policy<6>(epi, a);
        case 7: return v5_launch_policy<7>(epi, a);
        case 8: return v5_launch_policy<8>(epi, a);
        case 9: return v5_launch_policy<9>(epi, a);
    }
    set_error("v5 diag mode: bad mode / epilogue");
    return 1;
}

#endif   // POMS_V5_QUICK

// MODE 6 stamps: copy n u64 (<= kV5Stamps) to host (zeroed after the copy)
int kron_v5_stamps(unsigned long long* host, int64_t n) {
    if (n < 0 || n > kV5Stamps) { set_error("v5 stamps: bad count"); return 1; }
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_v5_stamps), n * sizeof(unsigned long long)) != hipSuccess) {
        set_error("v5 stamps: copy failed");
        return 1;
    }
    std::vector<unsigned long long> z((size_t)n, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_v5_stamps), z.data(), n * sizeof(unsigned long long)) != hipSuccess) {
        set_error("v5 stamps: clear failed");
        return 1;
    }
    return 0;
}

}  // namespace poms
