// wide_chain_linalg.h — one chain's dense K x K fp64 linear algebra for 1 <= K <= 128, on the chain's wave(s), in the chain's scratch
// (LDS, or its block of device memory: the pointer types are template arguments).  The five routines of chain_linalg.h — same names,
// argument order, layouts and aliasing rules — in a form whose registers and code do not grow with K: no per-lane array sized by K, no
// loop over K unrolled in full; what is unrolled is a fixed panel of PANEL = 32 columns (rows).  Included by the generated densities
// whose matrix stages are wider than chain_linalg.h takes (Model.compile(wide_matrices=True)); nothing else includes it.
//
// Layout: matrices are row-major, element (i, j) of a K x K matrix at i K + j; a K x N block of right-hand sides at i N + c.  Called by
// all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W)); every routine returns after the chain's barrier: its output is
// then visible to every lane.  The input arrays are not written.
//
// Order contract (DESIGN.md §11.5, to the letter): every dot product is ONE accumulator updated by fused multiply-adds in ascending order
// of its index, starting from the value it is subtracted from (or +0.0).  The subtracted products enter as fma(-l, x, s): the sign on the
// first factor.  L[i][j] = (A[i][j] - sum_{k < j} L[i][k] L[j][k]) / L[j][j] with k = 0 .. j-1 ascending; the pivot's square root is taken
// once, one division per element (no reciprocal); a pivot that is not a positive finite number makes ALL of L NaN and returns false.
// x_i = (b_i - sum_{k < i} L[i][k] x_k) / L[i][i]; y_i = (g_i - sum_{k > i, ascending} L[k][i] y_k) / L[i][i]; solve_lower_adj_l negates
// AFTER the sum (a zero sum gives -0.0 on the triangle); cholesky_adj: P with 0.5 * s, the two in-place substitutions, the fold
// G[i][j] + G[j][i], +0.0 above the diagonal.  No atomics, no sums across lanes, no split of a summed range: the result is a function of
// (K, N) and the chain's own inputs, not of W and not of which lane computes an element.  Restated on the CPU as the test oracle's
// oracle_chain_cholesky, _solve_lower, _solve_lower_t, _solve_lower_adj_l, _cholesky_adj (K is a run-time argument there);
// tests/test_gpu_matrix_wide.py holds the five routines to that bit for bit at W = 1, 2, 4.
//
// How the work is spread.  cholesky is left-looking in panels of 32 columns: a lane owns the rows lane, lane + 64 W, ...; for a panel it
// carries a row's 32 accumulators through all earlier columns (k ascending; the panel's rows of L are read as broadcasts), then finishes
// the panel in registers.  The block of rows that holds the panel's pivots goes column by column with the chain's barrier (the pivot
// reaches the other lanes through L itself); the blocks below it read a finished triangle and need no barrier.  solve_lower is the same
// in rows: the partial sums of a panel's 32 rows over the earlier rows of X are spread element by element over ALL lanes (one right-hand
// side keeps 32 lanes busy), then a lane per column finishes the panel's triangle in registers.  solve_lower_t cannot be spread within a
// column: its contract sums k = i + 1 .. K - 1 ASCENDING, so row i's chain starts when y_{i+1} is known and row i + 1's chain has ended —
// the K (K - 1) / 2 fused multiply-adds of one column are one dependent chain, whoever runs them; lanes stride over the N columns.
#pragma once

#ifndef NPHIP_JIT_W
#define NPHIP_JIT_W 1
#endif

namespace nphip_lw {

constexpr int MAX_K = 128;
constexpr int PANEL = 32;              // columns (rows) finished in registers at a time: the only fully unrolled extent
constexpr int T = 64 * NPHIP_JIT_W;    // lanes of the chain

// acc[c] = A[i][j0 + c] - sum_{k < j0, ascending} L[i][k] L[j0 + c][k]: row i's accumulators of the panel at column j0, carried through
// all earlier columns.  (Columns past K - 1 repeat column K - 1: read inside the arrays, never stored.)
template <int K, class PA, class PL>
__device__ __forceinline__ void panel_sums(PA A, PL L, int i, int j0, double (&acc)[PANEL]) {
#pragma unroll
    for (int c = 0; c < PANEL; ++c) acc[c] = A[i * K + (j0 + c < K ? j0 + c : K - 1)];
#pragma unroll 2
    for (int k = 0; k < j0; ++k) {
        const double lik = L[i * K + k];
#pragma unroll
        for (int c = 0; c < PANEL; ++c) acc[c] = __builtin_fma(-lik, L[(j0 + c < K ? j0 + c : K - 1) * K + k], acc[c]);   // (a broadcast read)
    }
}

// L = chol(A), lower triangle of A read, upper triangle of L written as +0.0.
template <int K, class PA, class PL>
__device__ __forceinline__ bool cholesky(PA A, PL L, int lane) {
    static_assert(K >= 1 && K <= MAX_K, "one chain's matrix: K <= 128");
    for (int e = lane; e < K * K; e += T)
        if (e % K > e / K) L[e] = 0.0;
    bool ok = true;
#pragma unroll 1
    for (int j0 = 0; j0 < K; j0 += PANEL) {
        const int rb0 = j0 / T;     // the block of rows that holds the panel's pivots (32 divides 64 W: all of them)
        {
            const int i = lane + T * rb0;
            const bool mine = i >= j0 && i < K;
            double acc[PANEL], row[PANEL];
            panel_sums<K>(A, L, mine ? i : j0, j0, acc);
#pragma unroll
            for (int c = 0; c < PANEL; ++c) {
                const int j = j0 + c;
                if (j >= K) break;
                double s = acc[c];
#pragma unroll
                for (int cc = 0; cc < c; ++cc) s = __builtin_fma(-row[cc], L[j * K + j0 + cc], s);
                if (mine && i == j) L[j * K + j] = (s > 0.0 && s < __builtin_huge_val()) ? __builtin_sqrt(s) : __builtin_nan("");
                nphip_chain_barrier();
                const double r = L[j * K + j];      // (the same value in every lane of the chain: all of them leave together)
                if (r != r) {
                    ok = false;
                    break;
                }
                row[c] = s / r;
                if (mine && i > j) L[i * K + j] = row[c];
                nphip_chain_barrier();
            }
        }
        if (!ok) break;
        // the blocks of rows below: against the panel's finished triangle
#pragma unroll 1
        for (int rb = rb0 + 1; rb * T < K; ++rb) {
            const int i = lane + T * rb;
            const bool mine = i < K;
            double acc[PANEL], row[PANEL];
            panel_sums<K>(A, L, mine ? i : j0, j0, acc);
#pragma unroll
            for (int c = 0; c < PANEL; ++c) {
                const int j = j0 + c;
                if (j >= K) break;
                double s = acc[c];
#pragma unroll
                for (int cc = 0; cc < c; ++cc) s = __builtin_fma(-row[cc], L[j * K + j0 + cc], s);
                row[c] = s / L[j * K + j];
                if (mine) L[i * K + j] = row[c];
            }
        }
        nphip_chain_barrier();
    }
    if (!ok) {
        nphip_chain_barrier();
        for (int e = lane; e < K * K; e += T) L[e] = __builtin_nan("");
        nphip_chain_barrier();
    }
    return ok;
}

// X = L^-1 B (forward substitution), B and X K x N.  X holds the partial sums of a panel's rows between the two steps.
template <int K, int N, class PL, class PB, class PX>
__device__ __forceinline__ void solve_lower(PL L, PB B, PX X, int lane) {
    static_assert(K >= 1 && K <= MAX_K && N >= 1, "");
#pragma unroll 1
    for (int j0 = 0; j0 < K; j0 += PANEL) {
        const int rows = K - j0 < PANEL ? K - j0 : PANEL;
        // s = b_i - sum_{k < j0} L[i][k] x_k for the panel's rows i and every column: an element per lane
        for (int e = lane; e < rows * N; e += T) {
            const int i = j0 + e / N, c = e % N;
            double s = B[i * N + c];
#pragma unroll 8
            for (int k = 0; k < j0; ++k) s = __builtin_fma(-L[i * K + k], X[k * N + c], s);
            X[i * N + c] = s;
        }
        nphip_chain_barrier();
        // the panel's triangle: a column per lane, its 32 x in registers
        for (int c = lane; c < N; c += T) {
            double x[PANEL];
#pragma unroll
            for (int r = 0; r < PANEL; ++r) {
                const int i = j0 + r;
                if (i >= K) break;
                double s = X[i * N + c];
#pragma unroll
                for (int q = 0; q < r; ++q) s = __builtin_fma(-L[i * K + j0 + q], x[q], s);
                x[r] = s / L[i * K + i];
                X[i * N + c] = x[r];
            }
        }
        nphip_chain_barrier();
    }
}

// Y = L^-T G (backward substitution with L^T), on the N "columns" of a K-row block whose element (i, c) is at i RS + c CS.  G and Y may
// be the same array (a lane reads an element of its column before it writes it).  The lane's y_k come back from Y.
template <int K, int N, int RS, int CS, class PL, class PG, class PY>
__device__ __forceinline__ void solve_lower_t(PL L, PG G, PY Y, int lane) {
    static_assert(K >= 1 && K <= MAX_K && N >= 1, "");
    for (int c = lane; c < N; c += T) {
#pragma unroll 1
        for (int i = K - 1; i >= 0; --i) {
            double s = G[i * RS + c * CS];
#pragma unroll 16
            for (int k = i + 1; k < K; ++k) s = __builtin_fma(-L[k * K + i], Y[k * RS + c * CS], s);   // (the loads do not wait for the chain: 32 in flight)
            Y[i * RS + c * CS] = s / L[i * K + i];
        }
    }
    nphip_chain_barrier();
}

// The adjoint of L in X = L^-1 B: Lbar = -tril(Bbar X^T).  Lanes stride over the K K elements; (i, j <= i) sums over the N columns in
// ascending order; the upper triangle is +0.0.
template <int K, int N, class PB, class PX, class PO>
__device__ __forceinline__ void solve_lower_adj_l(PB Bbar, PX X, PO Lbar, int lane) {
    static_assert(K >= 1 && K <= MAX_K && N >= 1, "");
    for (int e = lane; e < K * K; e += T) {
        const int i = e / K, j = e % K;
        double s = 0.0;
        if (j <= i) {
#pragma unroll 4
            for (int c = 0; c < N; ++c) s = __builtin_fma(Bbar[i * N + c], X[j * N + c], s);
            s = -s;
        }
        Lbar[e] = s;
    }
    nphip_chain_barrier();
}

// The adjoint of A in L = chol(A) (Murray 2016, arXiv:1602.07527), as chain_linalg.h states it: P = Phi(L^T Lbar) symmetrised,
// G = L^-T P L^-1 by the two backward substitutions in place, Abar = G folded onto the lower triangle.  Abar is the scratch of both.
template <int K, class PL, class PB, class PA>
__device__ __forceinline__ void cholesky_adj(PL L, PB Lbar, PA Abar, int lane) {
    static_assert(K >= 1 && K <= MAX_K, "");
    for (int e = lane; e < K * K; e += T) {
        const int i = e / K, j = e % K;
        if (j <= i) {
            double s = 0.0;
#pragma unroll 8
            for (int k = i; k < K; ++k) s = __builtin_fma(L[k * K + i], Lbar[k * K + j], s);
            const double p = 0.5 * s;
            Abar[i * K + j] = p;
            if (j != i) Abar[j * K + i] = p;
        }
    }
    nphip_chain_barrier();
    solve_lower_t<K, K, K, 1>(L, Abar, Abar, lane);   // L^-T P: the columns
    solve_lower_t<K, K, 1, K>(L, Abar, Abar, lane);   // (L^-T P) L^-1: the rows
    for (int e = lane; e < K * K; e += T) {            // below the diagonal: reads the upper triangle, writes the lower one
        const int i = e / K, j = e % K;
        if (j < i) Abar[e] = Abar[e] + Abar[j * K + i];
    }
    nphip_chain_barrier();
    for (int e = lane; e < K * K; e += T)
        if (e % K > e / K) Abar[e] = 0.0;
    nphip_chain_barrier();
}

}  // namespace nphip_lw
