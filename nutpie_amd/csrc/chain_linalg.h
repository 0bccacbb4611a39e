// chain_linalg.h — one chain's dense K x K fp64 linear algebra, on ONE wavefront, in the chain's scratch (LDS, or its block of
// device memory when the model's arrays do not fit the LDS).  Included by the generated densities that use the symbolic IR's
// matrix stages (nutpie_amd/symbolic.py: cholesky, solve_lower and their adjoints); nothing else includes it.
//
// Layout: matrices are row-major, element (i, j) of a K x K matrix at i K + j; a K x N block of right-hand sides at i N + c.
// Every routine is called by all 64 lanes of the chain's wave and returns after a wave barrier: its output is then visible to
// every lane.  The input arrays are not written.  The lane's own row (Cholesky) or column (substitutions) lives in registers;
// the other operand is read by broadcast loads — every active lane the same address.
//
// Summation order: every dot product is ONE accumulator updated by fused multiply-adds in ascending order of
// its index, starting from the value it is subtracted from (or +0.0).  No atomics and no cross-lane sums: a lane's results
// depend on its own chain only.  The subtracted products enter as fma(-l, x, s): the sign on the first factor.  Everything else is one
// IEEE operation per written operation: the pivot's square root, one division per element (no reciprocal), the halving and the
// fold G[i][j] + G[j][i] of cholesky_adj, the negation AFTER the sum in solve_lower_adj_l (a zero sum gives -0.0 on the triangle).
// Restated on the CPU as the test oracle's oracle_chain_cholesky, _solve_lower, _solve_lower_t, _solve_lower_adj_l, _cholesky_adj;
// tests/test_gpu_chain_stages.py holds the five routines to that bit for bit.
#pragma once

#if defined(NPHIP_JIT_W) && NPHIP_JIT_W != 1
#error "chain_linalg.h: the matrix stages run on one wavefront per chain (compile(waves_per_chain=1))"
#endif

namespace nphip_la {

// stores of some lanes visible to the loads of the others (the chain's wave; LDS or device memory)
__device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// L = chol(A), lower triangle of A read, upper triangle of L written as +0.0.  Column j: lane i >= j forms
// s_i = A[i][j] - sum_{k < j} L[i][k] L[j][k]; the pivot s_j reaches every lane by a cross-lane read.  A pivot that is not a
// positive finite number makes ALL of L NaN (the density is then NaN: an impossible point, a divergence for the sampler).
// Returns false then.
template <int K, class PA, class PL>
__device__ __forceinline__ bool cholesky(PA A, PL L, int lane) {
    static_assert(K >= 1 && K <= 32, "one chain's matrix: K <= 32");
    const int i = lane;
    for (int e = lane; e < K * K; e += 64)
        if (e % K > e / K) L[e] = 0.0;
    double row[K];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double s = 0.0;
        if (i >= j && i < K) {
            s = A[i * K + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = __builtin_fma(-row[k], L[j * K + k], s);
        }
        const double d = __shfl(s, j, 64);
        if (!(d > 0.0) || !(d < __builtin_huge_val())) {   // (the same value in every lane: the whole wave leaves)
            ok = false;
            break;
        }
        const double r = __builtin_sqrt(d);
        row[j] = (i == j) ? r : s / r;
        if (i >= j && i < K) L[i * K + j] = row[j];
        sync();
    }
    if (!ok) {
        sync();
        for (int e = lane; e < K * K; e += 64) L[e] = __builtin_nan("");
    }
    sync();
    return ok;
}

// X = L^-1 B (forward substitution), B and X K x N; lanes stride over the N columns.  x_i = (b_i - sum_{k < i} L[i][k] x_k) / L[i][i].
template <int K, int N, class PL, class PB, class PX>
__device__ __forceinline__ void solve_lower(PL L, PB B, PX X, int lane) {
    for (int c = lane; c < N; c += 64) {
        // (L is read again in every pass: hoisted out of the loop, its K (K + 1) / 2 elements would live in registers — spills at K = 32)
        asm volatile("" ::: "memory");
        double x[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double s = B[i * N + c];
#pragma unroll
            for (int k = 0; k < i; ++k) s = __builtin_fma(-L[i * K + k], x[k], s);
            x[i] = s / L[i * K + i];
            X[i * N + c] = x[i];
            asm volatile("" ::: "memory");   // (one row of L in flight at a time: the unrolled rows would all be loaded up front)
        }
    }
    sync();
}

// Y = L^-T G (backward substitution with L^T), on the N "columns" of a K-row block whose element (i, c) is at i RS + c CS;
// y_i = (g_i - sum_{k > i, ascending} L[k][i] y_k) / L[i][i].  G and Y may be the same array (a lane reads its column first).
template <int K, int N, int RS, int CS, class PL, class PG, class PY>
__device__ __forceinline__ void solve_lower_t(PL L, PG G, PY Y, int lane) {
    for (int c = lane; c < N; c += 64) {
        asm volatile("" ::: "memory");   // (as in solve_lower: L is not kept in registers across passes)
        double y[K];
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            double s = G[i * RS + c * CS];
#pragma unroll
            for (int k = i + 1; k < K; ++k) s = __builtin_fma(-L[k * K + i], y[k], s);
            y[i] = s / L[i * K + i];
            Y[i * RS + c * CS] = y[i];
            asm volatile("" ::: "memory");
        }
    }
    sync();
}

// The adjoint of L in X = L^-1 B: Lbar = -tril(Bbar X^T), with Bbar = L^-T Xbar (solve_lower_t).  Lanes stride over the K K
// elements; (i, j <= i) sums over the N columns in ascending order; the upper triangle is +0.0.
template <int K, int N, class PB, class PX, class PO>
__device__ __forceinline__ void solve_lower_adj_l(PB Bbar, PX X, PO Lbar, int lane) {
    for (int e = lane; e < K * K; e += 64) {
        const int i = e / K, j = e % K;
        double s = 0.0;
        if (j <= i) {
            for (int c = 0; c < N; ++c) s = __builtin_fma(Bbar[i * N + c], X[j * N + c], s);
            s = -s;
        }
        Lbar[e] = s;
    }
    sync();
}

// The adjoint of A in L = chol(A) (Murray 2016, arXiv:1602.07527):
//     P = Phi(L^T Lbar) symmetrised — 1/2 (L^T Lbar)[i][j] at (i, j) and (j, i) for i >= j (only the lower triangle of Lbar counts);
//     G = L^-T P L^-1 — the backward substitution over the columns of P, then over the rows of the result: torch.autograd's
//         symmetric gradient;
//     Abar = G folded onto the triangle that cholesky() reads: G[i][j] + G[j][i] below the diagonal, G[i][i] on it, +0.0 above —
//         the exact gradient of what is evaluated, and the same parameter gradient as torch's for a symmetric A.
// (L^T Lbar)[i][j] = sum_{k = i .. K-1, ascending} L[k][i] Lbar[k][j].  Abar is the scratch of both substitutions.
template <int K, class PL, class PB, class PA>
__device__ __forceinline__ void cholesky_adj(PL L, PB Lbar, PA Abar, int lane) {
    for (int e = lane; e < K * K; e += 64) {
        const int i = e / K, j = e % K;
        if (j <= i) {
            double s = 0.0;
            for (int k = i; k < K; ++k) s = __builtin_fma(L[k * K + i], Lbar[k * K + j], s);
            const double p = 0.5 * s;
            Abar[i * K + j] = p;
            if (j != i) Abar[j * K + i] = p;
        }
    }
    sync();
    solve_lower_t<K, K, K, 1>(L, Abar, Abar, lane);   // L^-T P: the columns
    solve_lower_t<K, K, 1, K>(L, Abar, Abar, lane);   // (L^-T P) L^-1: the rows
    for (int e = lane; e < K * K; e += 64) {            // below the diagonal: reads the upper triangle, writes the lower one
        const int i = e / K, j = e % K;
        if (j < i) Abar[e] = Abar[e] + Abar[j * K + i];
    }
    sync();
    for (int e = lane; e < K * K; e += 64)
        if (e % K > e / K) Abar[e] = 0.0;
    sync();
}

}  // namespace nphip_la
