// kalman_smoother.h — one chain's fixed-interval Kalman smoother: the mean and the variance of every state given ALL observations of its
// series, by the backward recursion of de Jong / Durbin & Koopman over what the filter stored (chain_kalman.h: forward).  Scalar
// observations: no matrix inverse, only divisions by the stored F.  Included by the generated expand functions that report
// nutpie_amd/symbolic.py: kalman_smoothed_state; a density never runs it (it carries no gradient), and nothing else includes it.
//
// Order contract (restated in plain C as tests/fixtures/kalman_smoother_reference.c — the normative text — and the
// routine is held to that bit for bit by tests/test_gpu_kalman_smoother_stages.py at W = 1, 2, 4).  dot_k(x, y) is s = +0.0, then
// s = fma(x_k, y_k, s) for ascending k = 0 .. m-1; every other written operation is one IEEE operation in the order written; every
// division is a true division, never a reciprocal.  Every output is a fixed function of (R, T, m, mask) and the chain's own inputs —
// not of W, the lane mapping, where the arrays live, or the form of the kernel; no atomics.
// Per series, from r = +0.0 (m) and N = +0.0 (m x m), for t = T-1 .. 0, with a = apred[t], P = Ppred[t], v = v[t], F = F[t], Z = Z[t]:
//   t < T-1:   u_k = dot_i(Tm[i][k], r_i);  V[k][j] = dot_i(Tm[i][k], N[i][j]);  W[k][l] = dot_j(V[k][j], Tm[j][l])
//   t = T-1:   u = +0.0, W = +0.0 (Tm is not read)
//   observed:  M_i = dot_k(P[i][.], Z);  K_i = M_i / F;  e = v / F - dot_k(K, u);  g_i = dot_j(W[i][.], K);  gt_j = dot_i(W[i][j], K_i);
//              D = 1.0 / F + dot_k(K, g);  r_k = fma(e, Z_k, u_k);
//              N[i][j] = fma(D * Z_i, Z_j, fma(-g_i, Z_j, fma(-Z_i, gt_j, W[i][j])))
//   missing:   r = u, N = W
//   asm[t]_i = a_i + dot_k(P[i][.], r);  Y[i][j] = dot_k(P[i][k], N[k][j]);  vsm[t]_i = P[i][i] - dot_j(Y[i][.], P[i][.])
// N and W are never symmetrised, and the last product reads row i of P where the algebra has column i: P is used as stored.
// Non-finite inputs are not guarded.  A NaN stays inside its series and inside its chain.
//
// Layout: as chain_kalman.h.  F is what `forward` stored, of which apred, Ppred, v and F are read; obs (R T; 0 = a missing observation)
// is read only with MASK.  The result is packed:  S = [ asm: R T m | vsm: R T m ]  — the smoothed mean of the state and the diagonal
// of its smoothed covariance.  On trailing missing steps these are the predicted mean and the diagonal of Ppred: a forecast.
// Called by all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W)); returns after the chain's barrier.  The inputs
// are not written.
//
// Lanes: those of `backward`.  G = the smallest power of two >= m adjacent lanes own one series, lane g G + i holding r_i and row i
// of N in registers; series r belongs to group r mod (64 W / G) in pass r div (64 W / G), a lane carries U passes at once.  Column i
// of Tm is read once, Tm (for W) and Z[t] by broadcast loads; rows of N and W and the elements of K, u, g, r arrive by cross-lane
// moves inside the group.  Nothing crosses a group.  A group without a series, and the lanes of a group beyond m, repeat work of
// series 0 resp. row 0 and store nothing.  A step is computed as if observed and the result selected: no lane leaves the step's
// cross-lane moves.
#pragma once

#include "chain_kalman.h"

namespace nphip_kalman {

template <int R, int T, int M, bool MASK, class PO, class PZ, class PT, class PF, class PS>
__device__ __forceinline__ void smooth(PO obs, PZ Z, PT Tm, PF F, PS Sm, int lane) {
    static_assert(R >= 1 && T >= 1 && M >= 1 && M <= MAX_STATE, "");
    constexpr int G = group_lanes(M), S = 64 * NPHIP_JIT_W / G, PASSES = (R + S - 1) / S, U = passes_at_once(M);
    const int l = lane & 63, g = lane / G;
    const bool row = (lane & (G - 1)) < M;
    const int i = row ? (lane & (G - 1)) : 0;
    const auto Apred = F;
    const auto Ppred = Apred + R * T * M;
    const auto Vs = Ppred + R * T * M * M + R * T * M;
    const auto Fs = Vs + R * T;
    const auto Asm = Sm;
    const auto Vsm = Asm + R * T * M;
    double Tc[M];      // column i of Tm
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if constexpr (T > 1) Tc[k] = (double)Tm[k * M + i];
        else Tc[k] = 0.0;
    }
    for (int p0 = 0; p0 < PASSES; p0 += U) {
        int r[U];
        bool act[U];
        double rr[U], N[U][M];     // r_i; row i of N
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int series = (p0 + u) * S + g;
            act[u] = row && series < R;
            r[u] = series < R ? series : 0;
            rr[u] = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) N[u][k] = 0.0;
        }
        for (int t = T - 1; t >= 0; --t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = r[u] * T + t;
                double z[M], P[M], W[M], Kv[M], uv[M], gv[M], gt[M], rv[M], Y[M];
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    z[k] = (double)Z[s * M + k];
                    P[k] = (double)Ppred[(s * M + i) * M + k];
                    gt[k] = 0.0;
                    Y[k] = 0.0;
                }
                const double zi = (double)Z[s * M + i], a = (double)Apred[s * M + i], Pii = (double)Ppred[(s * M + i) * M + i];
                const double v = (double)Vs[s], Fv = (double)Fs[s];
                bool seen = true;
                if constexpr (MASK) seen = (double)obs[s] != 0.0;
                double ui;
                if (t < T - 1) {
                    double V[M];
                    gather<G, M>(rr[u], l, rv);
                    ui = dot<M>(Tc, rv);
#pragma unroll
                    for (int j = 0; j < M; ++j) V[j] = 0.0;
                    // row i of V = Tm^T N: the rows i' of N in ascending order
                    each<0, M>([&](auto ip) {
                        constexpr int I = decltype(ip)::v;
                        double w[M];
                        row_of<G, I, M>(N[u], l, w);
#pragma unroll
                        for (int j = 0; j < M; ++j) V[j] = __builtin_fma(Tc[I], w[j], V[j]);
                    });
#pragma unroll
                    for (int q = 0; q < M; ++q) {
                        double s1 = 0.0;
#pragma unroll
                        for (int j = 0; j < M; ++j) s1 = __builtin_fma(V[j], (double)Tm[j * M + q], s1);
                        W[q] = s1;
                    }
                } else {
                    ui = 0.0;
#pragma unroll
                    for (int j = 0; j < M; ++j) W[j] = 0.0;
                }
                const double K = dot<M>(P, z) / Fv;
                gather<G, M>(K, l, Kv);
                gather<G, M>(ui, l, uv);
                const double e = v / Fv - dot<M>(Kv, uv);
                const double gi = dot<M>(W, Kv);
                // gt_j = dot_i'(W[i'][j], K_i'): the rows i' of W
                each<0, M>([&](auto ip) {
                    constexpr int I = decltype(ip)::v;
                    double w[M];
                    row_of<G, I, M>(W, l, w);
#pragma unroll
                    for (int j = 0; j < M; ++j) gt[j] = __builtin_fma(w[j], Kv[I], gt[j]);
                });
                gather<G, M>(gi, l, gv);
                const double D = 1.0 / Fv + dot<M>(Kv, gv);
                const double Dz = D * zi;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double n = __builtin_fma(Dz, z[j], __builtin_fma(-gi, z[j], __builtin_fma(-zi, gt[j], W[j])));
                    N[u][j] = seen ? n : W[j];
                }
                rr[u] = seen ? __builtin_fma(e, zi, ui) : ui;
                gather<G, M>(rr[u], l, rv);
                const double mean = a + dot<M>(P, rv);
                // row i of Y = P N: the rows k of N
                each<0, M>([&](auto kp) {
                    constexpr int Kk = decltype(kp)::v;
                    double w[M];
                    row_of<G, Kk, M>(N[u], l, w);
#pragma unroll
                    for (int j = 0; j < M; ++j) Y[j] = __builtin_fma(P[Kk], w[j], Y[j]);
                });
                const double var = Pii - dot<M>(Y, P);
                if (act[u]) {
                    Asm[s * M + i] = mean;
                    Vsm[s * M + i] = var;
                }
            }
        }
    }
    nphip_chain_barrier();
}

}  // namespace nphip_kalman
