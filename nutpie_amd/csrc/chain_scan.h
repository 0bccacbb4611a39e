// chain_scan.h — one chain's first-order linear recurrences x_t = a_t x_{t-1} + b_t, on the chain's wave(s), in its scratch (LDS, or
// its block of device memory when the model's arrays do not fit the LDS).  Included by the generated densities that use the symbolic
// IR's scan stages (nutpie_amd/symbolic.py: linear_recurrence, cumsum and their adjoint); nothing else includes it.
//
// Layout: R independent rows of T elements, row-major (element (r, t) at r T + t).  Each row has its own initial value x_{-1}
// (one scalar for all rows, or an array of R).  The coefficient a is an array (one per element), one scalar, or the constant 1
// (a prefix sum: no multiplier carried).  Called by all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W));
// returns after the chain's barrier: the output is then visible to every lane.  The input arrays are not written.
//
// Order contract (restated on the CPU as the test oracle's oracle_chain_scan, and the routine is held to that
// bit for bit by tests/test_gpu_chain_stages.py): a row is cut into segments of 64 W consecutive elements, lane l of the chain holding
// element s 64 W + l.  Every element is the affine map (A, B): x -> A x + B, past the row's end the identity (1, 0) — scanned like any
// other element (it comes after every stored one).  In a segment:
//   1. each wave takes the inclusive scan of its 64 maps by the fixed pattern row_shr 1, 2, 4, 8 (within rows of 16 lanes), then
//      row_bcast 15 (into rows 1, 3) and row_bcast 31 (into rows 2, 3); composing an earlier map (A1, B1) into a later one (A2, B2)
//      gives (A2 A1, fma(A2, B1, B2)) — with a = 1, B2 + B1 —; a lane that has no partner in a step composes the identity as the
//      EARLIER map, (A 1, fma(A, 0.0, B)) resp. B + 0.0.  That is an operation, not a no-op: B = -0.0 becomes +0.0 (unless A < 0), and
//      a non-finite A makes B NaN;
//   2. (W > 1) the wave totals go through LDS and every wave composes, from the identity, the totals of the waves before it in
//      ascending order, each total as the LATER map: P = (1, 0), then P = (A_v A_P, fma(A_v, B_P, B_v)) for v = 0 .. w - 1 (wave 0
//      keeps the identity), and xin = fma(A_P, carry, B_P) — with a = 1, carry + B_P; in wave 0 that is fma(1.0, carry, 0.0) resp.
//      carry + 0.0.  With W = 1 there is no such step: xin = carry;
//   3. the carry (x at the previous segment's last element, lane 64 W - 1; the row's x_{-1} for the first segment) goes in last:
//      x = fma(A_lane, xin, B_lane) — with a = 1, xin + B_lane.
// Every operation is a fixed function of (R, T, W) and the chain's own inputs: no atomics, nothing from other chains.  A non-finite
// input makes the outputs that depend on it non-finite; an explosive |a| > 1 overflows whatever the order (not guarded).
//
// REV = true is the adjoint: lambda_t = fma(a_{t+1}, lambda_{t+1}, xbar_t), lambda_{T-1} = xbar_{T-1} — the same routine on the
// reversed row (logical element t is stored at T - 1 - t), the coefficients shifted by one and x_{-1} = 0.
#pragma once

#ifndef NPHIP_JIT_W
#define NPHIP_JIT_W 1
#endif

namespace nphip_scan {

// segments scanned side by side: their wave scans are independent, only the carries chain
constexpr int U = 4;
enum { A_ARRAY = 0, A_SCALAR = 1, A_ONE = 2 };
// (W > 1: the wave totals (A, B) of the U segments, two sets used in turn — one chain per workgroup then)
__shared__ double tot_[NPHIP_JIT_W > 1 ? 2 * U * NPHIP_JIT_W * 2 : 1];

// the value of the lane CTRL's DPP pattern names, or `edge` where this lane has no partner in the step (`has`, from the lane id: the
// DPP move itself writes every lane — no row mask, invalid sources read 0 — and the selection is a plain v_cndmask)
template <int CTRL>
__device__ __forceinline__ double from_lane(double x, bool has, double edge) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, true);
    return has ? __hiloint2double(hi, lo) : edge;
}

// one step of the wave scan for all U segments: the earlier map (from the partner lane) composed into this lane's
template <int CTRL, bool ONE>
__device__ __forceinline__ void step(double (&A)[U], double (&B)[U], bool has) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const double pb = from_lane<CTRL>(B[u], has, 0.0);
        if constexpr (ONE) {
            B[u] = B[u] + pb;
        } else {
            const double pa = from_lane<CTRL>(A[u], has, 1.0);
            B[u] = __builtin_fma(A[u], pb, B[u]);
            A[u] = A[u] * pa;
        }
    }
}

template <bool ONE>
__device__ __forceinline__ void wave_scan(double (&A)[U], double (&B)[U], int l) {   // l: the hardware lane (0 .. 63)
    step<0x111, ONE>(A, B, (l & 15) >= 1);   // row_shr:1
    step<0x112, ONE>(A, B, (l & 15) >= 2);   // row_shr:2
    step<0x114, ONE>(A, B, (l & 15) >= 4);   // row_shr:4
    step<0x118, ONE>(A, B, (l & 15) >= 8);   // row_shr:8
    step<0x142, ONE>(A, B, (l & 16) != 0);   // row_bcast:15, into rows 1 and 3
    step<0x143, ONE>(A, B, l >= 32);         // row_bcast:31, into rows 2 and 3
}

__device__ __forceinline__ double lane_f64(double x, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

// x = the recurrence over every row of B (A: the coefficients when AK == A_ARRAY, else a_s or 1; I: the R initial values when IROW,
// else i_s).  Pointers may be LDS or device memory.
template <int R, int T, int AK, bool REV, bool IROW, class PA, class PB, class PI, class PX>
__device__ __forceinline__ void linear_recurrence(PA Acoef, double a_s, PB Bin, PI Iin, double i_s, PX X, int lane) {
    static_assert(R >= 1 && T >= 1, "");
    constexpr int W = NPHIP_JIT_W, SEG = 64 * W;
    constexpr bool ONE = AK == A_ONE;
    const int wave = lane >> 6;
    int parity = 0;
    for (int r = 0; r < R; ++r) {
        double carry = REV ? 0.0 : (IROW ? (double)Iin[r] : i_s);
        for (int s0 = 0; s0 < T; s0 += U * SEG) {
            double A[U], B[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = s0 + u * SEG + lane;                  // logical element
                const int m = r * T + (REV ? T - 1 - t : t);        // where it is stored
                A[u] = 1.0;
                B[u] = 0.0;
                if (t < T) {
                    B[u] = Bin[m];
                    if constexpr (AK == A_ARRAY) A[u] = REV ? (t == 0 ? 0.0 : (double)Acoef[m + 1]) : (double)Acoef[m];
                    else if constexpr (AK == A_SCALAR) A[u] = (REV && t == 0) ? 0.0 : a_s;
                }
            }
            wave_scan<ONE>(A, B, lane & 63);
            if constexpr (W > 1) {
                double* tot = tot_ + parity * (U * W * 2);
                if ((lane & 63) == 63) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        tot[(u * W + wave) * 2] = A[u];
                        tot[(u * W + wave) * 2 + 1] = B[u];
                    }
                }
                nphip_chain_barrier();
                parity ^= 1;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double PA_ = 1.0, PB_ = 0.0, xin = 0.0;         // the waves before this one, ascending; then the carry
                    for (int w = 0; w < W; ++w) {
                        const double in_w = ONE ? carry + PB_ : __builtin_fma(PA_, carry, PB_);
                        if (w == wave) xin = in_w;
                        const double ta = tot[(u * W + w) * 2], tb = tot[(u * W + w) * 2 + 1];
                        if (w == W - 1) carry = ONE ? in_w + tb : __builtin_fma(ta, in_w, tb);   // (what the last lane of the last wave stores)
                        if constexpr (ONE) {
                            PB_ = PB_ + tb;
                        } else {
                            PB_ = __builtin_fma(ta, PB_, tb);
                            PA_ = ta * PA_;
                        }
                    }
                    const double x = ONE ? xin + B[u] : __builtin_fma(A[u], xin, B[u]);
                    const int t = s0 + u * SEG + lane;
                    if (t < T) X[r * T + (REV ? T - 1 - t : t)] = x;
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double x = ONE ? carry + B[u] : __builtin_fma(A[u], carry, B[u]);
                    const int t = s0 + u * SEG + lane;
                    if (t < T) X[r * T + (REV ? T - 1 - t : t)] = x;
                    carry = lane_f64(x, 63);
                }
            }
        }
    }
    nphip_chain_barrier();
}

}  // namespace nphip_scan
