// chain_matvec.h — one chain's products with a data matrix: E = X B (times) and C = X^T G (times_t), on the chain's wave(s).
// Included by the generated densities that use the symbolic IR's data-matrix stages (nutpie_amd/symbolic.py: `X @ beta` with a wide
// design matrix, `X.T @ g`, and each other's adjoint); nothing else includes it.
//
// X is n x K float data shared by every chain, read from device memory (L2): it is never staged into LDS.  The model keeps it twice,
// row-major (X[i K + c]) and transposed (Xt[c n + i]), so that in both products consecutive lanes read consecutive addresses.  The
// per-chain operands are row-major with R right-hand sides: B and C are K x R, E and G are n x R; they live in the chain's scratch
// (LDS, or its block of device memory — the pointer types are template arguments).  K and R are template arguments, n is the data's.
// Called by all 64 W lanes of the chain (W = NPHIP_JIT_W waves, `lane` in [0, 64 W)); returns after the chain's barrier: the output
// is then visible to every lane.  The inputs are not written.
//
// Order contract: every output element is ONE accumulator that starts at +0.0 and takes one explicit fma per
// summed index in ascending order — E[i][r] = fma(X[i][c], B[c][r], E[i][r]) for c = 0 .. K-1, C[c][r] = fma(X[i][c], G[i][r],
// C[c][r]) for i = 0 .. n-1.  No atomics, no sums across lanes, no split of the summed range, nothing from another chain: the result
// is a function of (n, K, R) and the chain's own inputs, not of W and not of which lane computes it.
// Restated on the CPU as the test oracle's oracle_chain_times / oracle_chain_times_t; tests/test_gpu_chain_stages.py holds both
// routines to that bit for bit at W = 1, 2, 4.
//
// Issue: a lane keeps several outputs side by side (ROWS row blocks in times; up to COLB column blocks in times_t, a lane with more
// goes over the rows once per group of COLB) and the loads of several summed indices in flight (the loops are unrolled by COLS
// resp. DEPTH): a lone wave per SIMD waits out every access otherwise.  In times_t with K < 64 W the lanes without a column idle.
#pragma once

#ifndef NPHIP_JIT_W
#define NPHIP_JIT_W 1
#endif

namespace nphip_mv {

constexpr int ROWS = 4;    // times: row blocks of 64 W rows a lane accumulates side by side
constexpr int COLS = 8;    // times: columns whose loads are issued together
constexpr int DEPTH = 8;   // times_t: rows whose loads are issued together
constexpr int COLB = 4;    // times_t: column blocks of 64 W columns a lane accumulates side by side

typedef const __attribute__((address_space(1))) double* gptr;   // the matrix: device memory (global loads, not flat ones)

// E = X B.  Lane owns rows i = lane, lane + 64 W, ...
template <int K, int R, class PB, class PE>
__device__ __forceinline__ void times(const double* Xt_, PB B, PE E, int n, int lane) {
    static_assert(K >= 1 && R >= 1 && R <= 16, "");
    constexpr int T = 64 * NPHIP_JIT_W;
    const gptr Xt = (gptr)Xt_;
    for (int i0 = lane; i0 < n; i0 += T * ROWS) {
        int j[ROWS];
        double acc[ROWS][R];
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const int i = i0 + T * u;
            j[u] = i < n ? i : 0;          // (rows past the end read row 0 and are not stored)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[u][r] = 0.0;
        }
#pragma unroll COLS
        for (int c = 0; c < K; ++c) {
            double x[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) x[u] = Xt[(size_t)c * n + j[u]];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double b = B[c * R + r];     // the same address in every lane: a broadcast read
#pragma unroll
                for (int u = 0; u < ROWS; ++u) acc[u][r] = __builtin_fma(x[u], b, acc[u][r]);
            }
        }
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const int i = i0 + T * u;
            if (i < n) {
#pragma unroll
                for (int r = 0; r < R; ++r) E[i * R + r] = acc[u][r];
            }
        }
    }
    nphip_chain_barrier();
}

// C = X^T G.  Lane owns columns c = lane, lane + 64 W, ...
template <int K, int R, class PG, class PC>
__device__ __forceinline__ void times_t(const double* X_, PG G, PC C, int n, int lane) {
    static_assert(K >= 1 && R >= 1 && R <= 16, "");
    constexpr int T = 64 * NPHIP_JIT_W;
    constexpr int CB = (K + T - 1) / T;      // column blocks per lane ...
    constexpr int NB = CB < COLB ? CB : COLB;   // ... NB of them side by side: one pass over the rows per group of NB
    const gptr X = (gptr)X_;
    for (int c0 = lane; c0 < K; c0 += T * NB) {
        int j[NB];
        double acc[NB][R];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int c = c0 + T * u;
            j[u] = c < K ? c : 0;          // (columns past the end read column 0 and are not stored)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[u][r] = 0.0;
        }
#pragma unroll DEPTH
        for (int i = 0; i < n; ++i) {
            double x[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) x[u] = X[(size_t)i * K + j[u]];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double g = G[i * R + r];     // the same address in every lane: a broadcast read
#pragma unroll
                for (int u = 0; u < NB; ++u) acc[u][r] = __builtin_fma(x[u], g, acc[u][r]);
            }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int c = c0 + T * u;
            if (c < K) {
#pragma unroll
                for (int r = 0; r < R; ++r) C[c * R + r] = acc[u][r];
            }
        }
    }
    nphip_chain_barrier();
}

}  // namespace nphip_mv
