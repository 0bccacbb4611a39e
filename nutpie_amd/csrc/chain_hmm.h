// chain_hmm.h — one chain's hidden Markov models: the scaled forward algorithm, its backward pass and the adjoint of the transition
// matrix, on the chain's wave(s), in its scratch (LDS, or its block of device memory when the model's arrays do not fit the LDS).
// Included by the generated densities that use the symbolic IR's HMM stages (nutpie_amd/symbolic.py: hmm_marginal_lpdf,
// hmm_state_prob and their gradient); nothing else includes it.
//
// Layout: R independent series of T steps with K states (K <= 16).  logE holds the log emission densities, row-major: element
// (r, t, k) at (r T + t) K + k.  P is K x K row-major (row i: the weights of the next state given state i; the rows need not sum to
// one), pi the K initial weights.  The results are packed:
//   F (forward)  = [ alpha: R T K | c: R T | m: R T ]                 alpha_t the filtered state probabilities, c_t the step's scale,
//                                                                    m_t the largest logE of the step
//   B (backward) = [ beta: R T K | w: R T K | Pbar: K K | pibar: K ]  beta_t the scaled backward variable, w_t = e_t beta_t / c_t,
//                                                                    Pbar / pibar the gradients of the value with respect to P / pi
// The value is sum_r sum_t (log c_t + m_t); its gradient with respect to logE[t][k] is alpha_t[k] beta_t[k].
// Every routine is called by all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W)) and returns after the chain's
// barrier: the output is then visible to every lane.  The inputs are not written.  `backward` reads what `forward` wrote,
// `transition_adjoint` what both wrote.
//
// Lanes (forward, backward): G = the smallest power of two >= K adjacent lanes own one series, lane g G + k holding state k — its
// column of P in registers in the forward pass, its row in the backward pass.  S = 64 W / G series run side by side: series r
// belongs to group r mod S in pass r div S, and a lane carries U passes at once (their recurrences are independent: one waits on
// its division while the other issues).  The other states' values arrive by cross-lane moves inside the group (DPP quad
// permutations up to G = 4, ds_bpermute above); nothing crosses a group, let alone a wave: the only barrier is the one at the end.
// A single series (R = 1) keeps one group of one wave busy; the other lanes idle.
// Lanes (transition_adjoint): lane p owns element p of [Pbar | pibar] and walks the stored alpha and w of every series.
//
// Order contract (restated in plain C as tests/fixtures/hmm_reference.c, and the routines are held to that bit for
// bit by tests/test_gpu_hmm_stages.py at W = 1, 2, 4).  Every output is a fixed function of (R, T, K) and the chain's own inputs —
// not of W, G, how many series ran side by side, or where the arrays live; no atomics, nothing from another chain or series.
// Per series, with exp / log the spec's (include/nphip_spec.h):
//   m_t       = logE[t][0], then for k = 1 .. K-1: m_t = (logE[t][k] > m_t || logE[t][k] != logE[t][k]) ? logE[t][k] : m_t
//               (a NaN, once met, stays)
//   e_t[k]    = nphip_exp(logE[t][k] - m_t)
//   a_0[j]    = pi[j] * e_0[j];   a_t[j] = acc * e_t[j] with acc = +0.0, then acc = fma(alpha_{t-1}[i], P[i][j], acc), i = 0 .. K-1
//   c_t       = +0.0, then c_t = c_t + a_t[j], j = 0 .. K-1
//   alpha_t[j] = a_t[j] / c_t                                    (one IEEE division, no reciprocal)
//   beta_{T-1}[i] = 1;   w_t[j] = (e_t[j] * beta_t[j]) / c_t
//   beta_{t-1}[i] = +0.0, then fma(P[i][j], w_t[j], .), j = 0 .. K-1
//   Pbar[i][j] = +0.0, then + s_r for r = 0 .. R-1, where s_r = +0.0, then fma(alpha_{t-1}[i], w_t[j], s_r) for t = 1 .. T-1
//   pibar[k]   = +0.0, then + w_0[k] of series r, r = 0 .. R-1
// Non-finite inputs are not guarded: a logE of -inf is an impossible state; a step whose states are all -inf (or one +inf) gives
// m - m = NaN, and that series' outputs from there on are NaN, like whatever a NaN reaches.  Pbar and pibar sum over the series;
// everything else of another series, and all of another chain, keeps its bits.
#pragma once

#ifndef NPHIP_JIT_W
#define NPHIP_JIT_W 1
#endif

namespace nphip_hmm {

constexpr int MAX_K = 16;
// passes (series of one group) a lane carries side by side
constexpr int U = 2;

constexpr int group_lanes(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

// compile-time loop: the DPP patterns are immediates
template <int I> struct at_ { static constexpr int v = I; };
template <int I, int N, class F>
__device__ __forceinline__ void each(F&& f) {
    if constexpr (I < N) {
        f(at_<I>{});
        each<I + 1, N>(f);
    }
}

// the value lane I of this lane's group of G holds (every lane of the wave takes part; `l` the hardware lane, 0 .. 63)
template <int G, int I>
__device__ __forceinline__ double from_group(double x, int l) {
    if constexpr (G == 1) {
        return x;
    } else if constexpr (G <= 4) {     // quad_perm: [I, I, I, I], resp. [I, I, 2 + I, 2 + I] for the two pairs of a quad
        constexpr int CTRL = G == 4 ? (I | (I << 2) | (I << 4) | (I << 6)) : (I | (I << 2) | ((2 + I) << 4) | ((2 + I) << 6));
        const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, true);
        const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, true);
        return __hiloint2double(hi, lo);
    } else {
        const int src = ((l & ~(G - 1)) | I) << 2;
        const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(x));
        const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(x));
        return __hiloint2double(hi, lo);
    }
}

template <int G, int K>
__device__ __forceinline__ void gather_group(double x, int l, double (&v)[K]) {
    each<0, K>([&](auto i) { v[decltype(i)::v] = from_group<G, decltype(i)::v>(x, l); });
}

// F = [alpha | c | m] of every series.  Lane g G + j: state j of the series of group g.
template <int R, int T, int K, class PE, class PP, class PI, class PF>
__device__ __forceinline__ void forward(PE logE, PP P, PI pi, PF F, int lane) {
    static_assert(R >= 1 && T >= 1 && K >= 1 && K <= MAX_K, "");
    constexpr int G = group_lanes(K), S = 64 * NPHIP_JIT_W / G, PASSES = (R + S - 1) / S;
    const int l = lane & 63, j = lane & (G - 1), g = lane / G;
    const bool state = j < K;
    const auto A = F;
    const auto C = F + R * T * K;
    const auto M = C + R * T;
    double Pc[K];      // column j
#pragma unroll
    for (int i = 0; i < K; ++i) Pc[i] = state ? (double)P[i * K + j] : 0.0;
    const double pj = state ? (double)pi[j] : 0.0;
    for (int p0 = 0; p0 < PASSES; p0 += U) {
        int r[U];
        bool act[U];
        double al[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r[u] = (p0 + u) * S + g;
            act[u] = state && r[u] < R;
        }
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int at = (r[u] * T + t) * K + j;
                const double le = act[u] ? (double)logE[at] : 0.0;
                double v[K];
                gather_group<G, K>(le, l, v);
                double m = v[0];
#pragma unroll
                for (int k = 1; k < K; ++k) m = (v[k] > m || v[k] != v[k]) ? v[k] : m;
                const double e = nphip_exp(le - m);
                double a;
                if (t == 0) {
                    a = pj * e;
                } else {
                    double acc = 0.0;
#pragma unroll
                    for (int i = 0; i < K; ++i) acc = __builtin_fma(al[u][i], Pc[i], acc);
                    a = acc * e;
                }
                gather_group<G, K>(a, l, v);
                double c = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) c = c + v[k];
                const double alpha = a / c;
                if (act[u]) {
                    A[at] = alpha;
                    if (j == 0) {
                        C[r[u] * T + t] = c;
                        M[r[u] * T + t] = m;
                    }
                }
                if (t + 1 < T) gather_group<G, K>(alpha, l, al[u]);
            }
        }
    }
    nphip_chain_barrier();
}

// B = [beta | w | . | .] of every series (Pbar and pibar: transition_adjoint).  Lane g G + i: state i of the series of group g.
template <int R, int T, int K, class PE, class PP, class PF, class PB>
__device__ __forceinline__ void backward(PE logE, PP P, PF F, PB B, int lane) {
    static_assert(R >= 1 && T >= 1 && K >= 1 && K <= MAX_K, "");
    constexpr int G = group_lanes(K), S = 64 * NPHIP_JIT_W / G, PASSES = (R + S - 1) / S;
    const int l = lane & 63, i = lane & (G - 1), g = lane / G;
    const bool state = i < K;
    const auto C = F + R * T * K;
    const auto M = C + R * T;
    const auto Bt = B;
    const auto Wt = B + R * T * K;
    double Pr[K];      // row i
#pragma unroll
    for (int k = 0; k < K; ++k) Pr[k] = state ? (double)P[i * K + k] : 0.0;
    for (int p0 = 0; p0 < PASSES; p0 += U) {
        int r[U];
        bool act[U];
        double beta[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r[u] = (p0 + u) * S + g;
            act[u] = state && r[u] < R;
            beta[u] = 1.0;
        }
        for (int t = T - 1; t >= 0; --t) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int at = (r[u] * T + t) * K + i;
                const double le = act[u] ? (double)logE[at] : 0.0;
                const double m = act[u] ? (double)M[r[u] * T + t] : 0.0;
                const double c = act[u] ? (double)C[r[u] * T + t] : 1.0;
                const double e = nphip_exp(le - m);
                const double w = (e * beta[u]) / c;
                if (act[u]) {
                    Bt[at] = beta[u];
                    Wt[at] = w;
                }
                if (t > 0) {
                    double v[K];
                    gather_group<G, K>(w, l, v);
                    double acc = 0.0;
#pragma unroll
                    for (int k = 0; k < K; ++k) acc = __builtin_fma(Pr[k], v[k], acc);
                    beta[u] = acc;
                }
            }
        }
    }
    nphip_chain_barrier();
}

// [Pbar | pibar] of B from the stored alpha (of F) and w (of B): lane p owns element p.
template <int R, int T, int K, class PF, class PB>
__device__ __forceinline__ void transition_adjoint(PF F, PB B, int lane) {
    static_assert(R >= 1 && T >= 1 && K >= 1 && K <= MAX_K, "");
    const auto A = F;
    const auto Wt = B + R * T * K;
    const auto Out = Wt + R * T * K;
    for (int p = lane; p < K * K + K; p += 64 * NPHIP_JIT_W) {
        double total = 0.0;
        if (p < K * K) {
            const int i = p / K, j = p % K;
            for (int r = 0; r < R; ++r) {
                double s = 0.0;
#pragma unroll 4
                for (int t = 1; t < T; ++t) s = __builtin_fma((double)A[(r * T + t - 1) * K + i], (double)Wt[(r * T + t) * K + j], s);
                total = total + s;
            }
        } else {
#pragma unroll 4
            for (int r = 0; r < R; ++r) total = total + (double)Wt[r * T * K + (p - K * K)];
        }
        Out[p] = total;
    }
    nphip_chain_barrier();
}

}  // namespace nphip_hmm
