// chain_kalman.h — one chain's linear Gaussian state-space models: the Kalman filter with the state summed out and the adjoint of the
// filter, on the chain's wave(s), in its scratch (LDS, or its block of device memory when the model's arrays do not fit the LDS).
// Included by the generated densities that use the symbolic IR's Kalman stages (nutpie_amd/symbolic.py: kalman_marginal_lpdf,
// kalman_filtered_state and their gradient); nothing else includes it.
//
// Order contract (restated in plain C as tests/fixtures/kalman_reference.c — the normative text — and the routines
// are held to that bit for bit by tests/test_gpu_kalman_stages.py at W = 1, 2, 4).  dot_k(x, y) is s = +0.0, then s = fma(x_k, y_k, s)
// for ascending k = 0 .. m-1; every other written operation is one IEEE operation in the order written; every division is a true
// division, never a reciprocal.  Every output is a fixed function of (R, T, m, mask) and the chain's own inputs — not of W, the lane
// mapping, where the arrays live, or the form of the kernel; no atomics.
// Forward, per series, from a = a0, P = P0, for t = 0 .. T-1:
//   apred[t] = a, Ppred[t] = P
//   observed:  v = y[t] - dot_k(Z[t], a);  M_i = dot_k(P[i][.], Z[t]);  F = h[t] + dot_k(Z[t], M);  K_i = M_i / F;
//              af_i = fma(K_i, v, a_i);  Pf[i][j] = fma(-K_i, M_j, P[i][j])
//   missing:   v = +0.0, F = 1.0, af = a, Pf = P
//   v[t] = v, F[t] = F, afilt[t] = af
//   t < T-1:   a_i = dot_k(Tm[i][.], af);  X[i][j] = dot_k(Pf[i][.], Tm[j][.]);  P[i][j] = Q[i][j] + dot_k(Tm[i][.], X[.][j])
// P is never symmetrised: every element is its own chain of operations, and the adjoint is that of what is evaluated.
// Backward, per series, from ab+ = 0, Pb+ = 0, Tb_r = Qb_r = +0.0, for t = T-1 .. 0 (vbar, Fbar: the adjoints of the stored v and F):
//   M, K, af, Pf again from the stored apred[t], Ppred[t], v[t], F[t]
//   t < T-1:   X again;  Qb_r[i][j] += Pb+[i][j];  Xb[k][j] = dot_i(Tm[i][k], Pb+[i][j]);
//              Tb_r[i][k] = ((Tb_r[i][k] + dot_j(Pb+[i][j], X[k][j])) + dot_l(Xb[l][i], Pf[l][k])) + ab+_i * af_k;
//              Pfb[i][k] = dot_j(Xb[i][j], Tm[j][k]);  afb_k = dot_i(Tm[i][k], ab+_i)           (else Pfb = 0, afb = 0)
//   observed:  Kb_i = afb_i * v - dot_j(Pfb[i][j], M_j);  vb = vbar[t] + dot_i(afb_i, K_i);  Mb_j = -dot_i(Pfb[i][j], K_i);
//              Mb_i = Mb_i + Kb_i / F;  Fb = Fbar[t] - dot_i(Kb_i, K_i) / F;  hbar[t] = Fb;  Mb_k = fma(Fb, Z_k, Mb_k);
//              Pb[i][k] = fma(Mb_i, Z_k, Pfb[i][k]);  Zbar[t][k] = (Fb * M_k + dot_i(P[i][k], Mb_i)) - vb * a_k;  ybar[t] = vb;
//              ab_k = fma(-vb, Z_k, afb_k)
//   missing:   ab = afb, Pb = Pfb, ybar = hbar = +0.0, Zbar[t] = +0.0
//   ab+ = ab, Pb+ = Pb;  after t = 0: a0b_r = ab+, P0b_r = Pb+
// Tbar, Qbar, a0bar, P0bar are each +0.0 + part_0 + part_1 + ... over ascending r, one lane per element, after a barrier.
// Non-finite inputs and F <= 0 are not guarded (the generated log F is then NaN: a divergence).  A NaN stays inside its series,
// except in the four sums over the series, and inside its chain.
//
// Layout: R independent series of T steps, state dimension m <= 8, one scalar observation per step.  All series share Tm (m x m
// row-major transition), Q (m x m state covariance), a0 (m) and P0 (m x m): the mean and covariance of the state at t = 0, before the
// first observation.  Per series and step: y (R T), Z (R T m: the design row of the step), h (R T: the observation variance), and
// with MASK obs (R T; 0 = a missing observation).  The results are packed:
//   F = [ apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T ]
//   B = [ ybar: R T | hbar: R T | Zbar: R T m | Tbar: m m | Qbar: m m | a0bar: m | P0bar: m m |
//         per-series partials: R x (Tb: m m | Qb: m m | a0b: m | P0b: m m) ]
// Every routine is called by all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W)) and returns after the chain's
// barrier.  The inputs are not written.  `backward` reads what `forward` wrote.
//
// Lanes: G = the smallest power of two >= m adjacent lanes own one series, lane g G + i holding row i of the covariance (of its
// adjoint in the backward pass: row i and column i) and element i of the mean in registers.  S = 64 W / G series run side by side:
// series r belongs to group r mod S in pass r div S, and a lane carries U passes at once (U = 2 up to m = 4: one series' division
// overlaps the other's fma chains; 1 above, where two sets of rows would not fit the registers).  Tm, Q and Z[t] are read by
// broadcast loads (every lane of a group reads the same address); the other rows' values arrive by cross-lane moves inside the group
// (DPP quad permutations up to G = 4, ds_bpermute for G = 8).  Nothing crosses a group before the final sum.  A group without a
// series, and the lanes of a group beyond m, repeat work of series 0 resp. row 0 and store nothing.
// A single series (R = 1) keeps one group of one wave busy; the other lanes idle: the recurrence is sequential in t.
#pragma once

#include "chain_hmm.h"      // from_group / each: the cross-lane moves inside a group

namespace nphip_kalman {

constexpr int MAX_STATE = 8;

constexpr int group_lanes(int M) { return nphip_hmm::group_lanes(M); }
// passes (series of one group) a lane carries side by side
constexpr int passes_at_once(int M) { return M <= 4 ? 2 : 1; }

using nphip_hmm::each;
using nphip_hmm::from_group;

// v[k] = x of lane k of the group
template <int G, int M>
__device__ __forceinline__ void gather(double x, int l, double (&v)[M]) {
    each<0, M>([&](auto k) { v[decltype(k)::v] = from_group<G, decltype(k)::v>(x, l); });
}

// v[j] = x[j] of lane I of the group: row I of a matrix kept by rows
template <int G, int I, int M>
__device__ __forceinline__ void row_of(const double (&x)[M], int l, double (&v)[M]) {
#pragma unroll
    for (int j = 0; j < M; ++j) v[j] = from_group<G, I>(x[j], l);
}

template <int M>
__device__ __forceinline__ double dot(const double (&x)[M], const double (&y)[M]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) s = __builtin_fma(x[k], y[k], s);
    return s;
}

// the measurement update of lane i's row from the predicted a_i, P[i][.], M_i and all of M: K_i, af_i, Pf[i][.]
template <int M>
__device__ __forceinline__ void update(bool seen, double a, const double (&P)[M], double v, double Fv, double Mi, const double (&Mv)[M], double& K,
                                       double& af, double (&Pf)[M]) {
    K = Mi / Fv;
    af = seen ? __builtin_fma(K, v, a) : a;
#pragma unroll
    for (int j = 0; j < M; ++j) Pf[j] = seen ? __builtin_fma(-K, Mv[j], P[j]) : P[j];
}

// X[i][j] = dot_k(Pf[i][.], Tm[j][.]) of lane i's row; Tm by broadcast loads
template <int M, class PT>
__device__ __forceinline__ void times_transposed(const double (&Pf)[M], PT Tm, double (&X)[M]) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) s = __builtin_fma(Pf[k], (double)Tm[j * M + k], s);
        X[j] = s;
    }
}

template <int R, int T, int M, bool MASK, class PY, class PO, class PZ, class PH, class PT, class PQ, class PA, class PP, class PF>
__device__ __forceinline__ void forward(PY y, PO obs, PZ Z, PH h, PT Tm, PQ Q, PA a0, PP P0, PF F, int lane) {
    static_assert(R >= 1 && T >= 1 && M >= 1 && M <= MAX_STATE, "");
    constexpr int G = group_lanes(M), S = 64 * NPHIP_JIT_W / G, PASSES = (R + S - 1) / S, U = passes_at_once(M);
    const int l = lane & 63, g = lane / G;
    const bool row = (lane & (G - 1)) < M;
    const int i = row ? (lane & (G - 1)) : 0;
    const auto Apred = F;
    const auto Ppred = Apred + R * T * M;
    const auto Afilt = Ppred + R * T * M * M;
    const auto Vs = Afilt + R * T * M;
    const auto Fs = Vs + R * T;
    double Tr[M], Qr[M];     // row i
#pragma unroll
    for (int k = 0; k < M; ++k) {
        Tr[k] = (double)Tm[i * M + k];
        Qr[k] = (double)Q[i * M + k];
    }
    for (int p0 = 0; p0 < PASSES; p0 += U) {
        int r[U];
        bool act[U];
        double a[U], P[U][M];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int series = (p0 + u) * S + g;
            act[u] = row && series < R;
            r[u] = series < R ? series : 0;
            a[u] = (double)a0[i];
#pragma unroll
            for (int k = 0; k < M; ++k) P[u][k] = (double)P0[i * M + k];
        }
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = r[u] * T + t;
                double z[M], av[M], Mv[M], Pf[M];
#pragma unroll
                for (int k = 0; k < M; ++k) z[k] = (double)Z[s * M + k];
                bool seen = true;
                if constexpr (MASK) seen = (double)obs[s] != 0.0;
                if (act[u]) {
                    Apred[s * M + i] = a[u];
#pragma unroll
                    for (int k = 0; k < M; ++k) Ppred[(s * M + i) * M + k] = P[u][k];
                }
                gather<G, M>(a[u], l, av);
                double v = (double)y[s] - dot<M>(z, av);
                const double Mi = dot<M>(P[u], z);
                gather<G, M>(Mi, l, Mv);
                double Fv = (double)h[s] + dot<M>(z, Mv);
                if (!seen) {
                    v = 0.0;
                    Fv = 1.0;
                }
                double K, af;
                update<M>(seen, a[u], P[u], v, Fv, Mi, Mv, K, af, Pf);
                if (act[u]) {
                    Afilt[s * M + i] = af;
                    if (i == 0) {
                        Vs[s] = v;
                        Fs[s] = Fv;
                    }
                }
                if (t < T - 1) {
                    double afv[M], X[M], Xc[M];
                    gather<G, M>(af, l, afv);
                    a[u] = dot<M>(Tr, afv);
                    times_transposed<M>(Pf, Tm, X);
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        gather<G, M>(X[j], l, Xc);     // column j of X
                        P[u][j] = Qr[j] + dot<M>(Tr, Xc);
                    }
                }
            }
        }
    }
    nphip_chain_barrier();
}

template <int R, int T, int M, bool MASK, class PY, class PO, class PZ, class PH, class PT, class PQ, class PF, class PV, class PG, class PB>
__device__ __forceinline__ void backward(PY y, PO obs, PZ Z, PH h, PT Tm, PQ Q, PF F, PV vbar, PG Fbar, PB B, int lane) {
    static_assert(R >= 1 && T >= 1 && M >= 1 && M <= MAX_STATE, "");
    constexpr int G = group_lanes(M), S = 64 * NPHIP_JIT_W / G, PASSES = (R + S - 1) / S, U = passes_at_once(M);
    constexpr int PS = 3 * M * M + M;     // one series' partials: Tb | Qb | a0b | P0b
    const int l = lane & 63, g = lane / G;
    const bool row = (lane & (G - 1)) < M;
    const int i = row ? (lane & (G - 1)) : 0;
    const auto Apred = F;
    const auto Ppred = Apred + R * T * M;
    const auto Vs = Ppred + R * T * M * M + R * T * M;
    const auto Fs = Vs + R * T;
    const auto Yb = B;
    const auto Hb = Yb + R * T;
    const auto Zb = Hb + R * T;
    const auto Sums = Zb + R * T * M;     // Tbar | Qbar | a0bar | P0bar, in the partials' order
    const auto Part = Sums + PS;
    (void)y; (void)h; (void)Q;
    double Tc[M];      // column i of Tm
#pragma unroll
    for (int k = 0; k < M; ++k) Tc[k] = (double)Tm[k * M + i];
    for (int p0 = 0; p0 < PASSES; p0 += U) {
        int r[U];
        bool act[U];
        double ab[U], Pbr[U][M], Pbc[U][M], Tb[U][M], Qb[U][M];     // ab+_i; row i and column i of Pb+; row i of Tb_r and Qb_r
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int series = (p0 + u) * S + g;
            act[u] = row && series < R;
            r[u] = series < R ? series : 0;
            ab[u] = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) Pbr[u][k] = Pbc[u][k] = Tb[u][k] = Qb[u][k] = 0.0;
        }
        for (int t = T - 1; t >= 0; --t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = r[u] * T + t;
                double z[M], P[M], Pcol[M], Mv[M], Pf[M], Pfbr[M], Pfbc[M];
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    z[k] = (double)Z[s * M + k];
                    P[k] = (double)Ppred[(s * M + i) * M + k];
                    Pcol[k] = (double)Ppred[(s * M + k) * M + i];
                }
                const double zi = (double)Z[s * M + i], a = (double)Apred[s * M + i], v = (double)Vs[s], Fv = (double)Fs[s];
                bool seen = true;
                if constexpr (MASK) seen = (double)obs[s] != 0.0;
                const double Mi = dot<M>(P, z);
                gather<G, M>(Mi, l, Mv);
                double K, af, afb;
                update<M>(seen, a, P, v, Fv, Mi, Mv, K, af, Pf);
                if (t < T - 1) {
                    double X[M], Xb[M], Xbc[M], afv[M], abv[M], t1[M], t2[M];
                    times_transposed<M>(Pf, Tm, X);
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        Qb[u][j] = Qb[u][j] + Pbr[u][j];
                        Xb[j] = 0.0;
                        t2[j] = 0.0;
                        Pfbc[j] = 0.0;
                    }
                    // row i of Xb: Xb[i][j] = dot_i'(Tm[i'][i], Pb+[i'][j]), the rows i' of Pb+ in ascending order
                    each<0, M>([&](auto ip) {
                        constexpr int I = decltype(ip)::v;
                        double w[M];
                        row_of<G, I, M>(Pbr[u], l, w);
#pragma unroll
                        for (int j = 0; j < M; ++j) Xb[j] = __builtin_fma(Tc[I], w[j], Xb[j]);
                    });
                    // column i of Xb: Xb[k][i] = dot_i'(Tm[i'][k], Pb+[i'][i])
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        double s1 = 0.0;
#pragma unroll
                        for (int q = 0; q < M; ++q) s1 = __builtin_fma((double)Tm[q * M + k], Pbc[u][q], s1);
                        Xbc[k] = s1;
                    }
                    // dot_j(Pb+[i][j], X[k][j]): the rows k of X
                    each<0, M>([&](auto kp) {
                        constexpr int Kk = decltype(kp)::v;
                        double w[M];
                        row_of<G, Kk, M>(X, l, w);
                        t1[Kk] = dot<M>(Pbr[u], w);
                    });
                    // dot_l(Xb[l][i], Pf[l][k]) over the rows l of Pf; column i of Pfb: Pfb[l][i] = dot_j(Xb[l][j], Tm[j][i]) from the rows l of Xb
                    each<0, M>([&](auto lp) {
                        constexpr int L = decltype(lp)::v;
                        double w[M], x[M];
                        row_of<G, L, M>(Pf, l, w);
#pragma unroll
                        for (int k = 0; k < M; ++k) t2[k] = __builtin_fma(Xbc[L], w[k], t2[k]);
                        row_of<G, L, M>(Xb, l, x);
                        Pfbc[L] = dot<M>(x, Tc);
                    });
                    gather<G, M>(af, l, afv);
#pragma unroll
                    for (int k = 0; k < M; ++k) Tb[u][k] = ((Tb[u][k] + t1[k]) + t2[k]) + ab[u] * afv[k];
                    // row i of Pfb: Pfb[i][k] = dot_j(Xb[i][j], Tm[j][k])
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        double s1 = 0.0;
#pragma unroll
                        for (int j = 0; j < M; ++j) s1 = __builtin_fma(Xb[j], (double)Tm[j * M + k], s1);
                        Pfbr[k] = s1;
                    }
                    gather<G, M>(ab[u], l, abv);
                    afb = dot<M>(Tc, abv);
                } else {
#pragma unroll
                    for (int k = 0; k < M; ++k) Pfbr[k] = Pfbc[k] = 0.0;
                    afb = 0.0;
                }
                if (seen) {
                    double Kv[M], afbv[M], Kbv[M], Mbv[M];
                    const double Kb = afb * v - dot<M>(Pfbr, Mv);
                    gather<G, M>(K, l, Kv);
                    gather<G, M>(afb, l, afbv);
                    const double vb = (double)vbar[s] + dot<M>(afbv, Kv);
                    double Mb = -dot<M>(Pfbc, Kv);
                    Mb = Mb + Kb / Fv;
                    gather<G, M>(Kb, l, Kbv);
                    const double Fb = (double)Fbar[s] - dot<M>(Kbv, Kv) / Fv;
                    Mb = __builtin_fma(Fb, zi, Mb);
                    gather<G, M>(Mb, l, Mbv);
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        Pbr[u][k] = __builtin_fma(Mb, z[k], Pfbr[k]);
                        Pbc[u][k] = __builtin_fma(Mbv[k], zi, Pfbc[k]);
                    }
                    const double zb = (Fb * Mi + dot<M>(Pcol, Mbv)) - vb * a;
                    ab[u] = __builtin_fma(-vb, zi, afb);
                    if (act[u]) {
                        Zb[s * M + i] = zb;
                        if (i == 0) {
                            Yb[s] = vb;
                            Hb[s] = Fb;
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        Pbr[u][k] = Pfbr[k];
                        Pbc[u][k] = Pfbc[k];
                    }
                    ab[u] = afb;
                    if (act[u]) {
                        Zb[s * M + i] = 0.0;
                        if (i == 0) {
                            Yb[s] = 0.0;
                            Hb[s] = 0.0;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (act[u]) {
                const auto mine = Part + r[u] * PS;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    mine[i * M + k] = Tb[u][k];
                    mine[M * M + i * M + k] = Qb[u][k];
                    mine[2 * M * M + M + i * M + k] = Pbr[u][k];
                }
                mine[2 * M * M + i] = ab[u];
            }
        }
    }
    nphip_chain_barrier();
    // the sums over the series: one lane per element, ascending r
    for (int e = lane; e < PS; e += 64 * NPHIP_JIT_W) {
        double total = 0.0;
#pragma unroll 4
        for (int q = 0; q < R; ++q) total = total + (double)Part[q * PS + e];
        Sums[e] = total;
    }
    nphip_chain_barrier();
}

}  // namespace nphip_kalman
