// nutpie-hip: the window estimator of adaptation="low_rank" as one kernel, WIDE shape (include/nutpie_hip.h: nphip_low_rank_estimate_wide):
// up to 1024 dimensions and 64 basis draws, i.e. a subspace problem of order R = 128 — what low_rank.basis_draws_for asks for above 256
// dimensions, which lowrank_est.hip (R = 64, four R x R matrices in LDS) does not cover.  lowrank_est.hip's header comment has the
// estimator itself; lowrank_est_common.h has the contract both kernels keep and the code they share.
//
// What is different: ONE R x R matrix lives in LDS at a time (column stride 130: 133 120 B of the CU's 163 840), everything else is parked
// in a per-workgroup block of device memory (L2-resident), and neither eigenproblem is formed as a symmetric matrix.  With Cg = Rc Rc' and
// Cx = Lx Lx' (Cholesky; both >= gamma I),
//     F1 = Rc' Lx                      F1 F1' = Rc' Cx Rc = U S^2 U'
//     one-sided Jacobi on the columns of F1 (rotations not accumulated): column j -> u_j s_j
//     scale column j by s_j^-1/2, solve Rc' F2 = U S^1/2 in place:      F2 F2' = Rc^-T (Rc' Cx Rc)^1/2 Rc^-1 = S, the geometric mean
//     one-sided Jacobi on the columns of F2: column j -> w_j e_j^1/2    (e_j: the spectrum of S, w_j: its eigenvectors, in Q's coordinates)
// — the condition number of what Jacobi sees is the square root of the explicit product's, and one matrix is rotated instead of two.
// The steps, one workgroup of 1024 threads per chain (or several chains in turn):
//   A moments -> device scratch;  B Gram matrix Z Z' (32-dimension tiles staged inside the matrix area, a 4 x 4 register block per thread);
//   C pivoted Cholesky in place, L parked;  E Cx, Cg from the rows of L in registers -> scratch;  F Cholesky of Cg (parked), of Cx, F1 in
//   registers -> LDS;  H Jacobi;  I scaling and back substitution with Rc read from scratch;  J Jacobi;  L selection (128 threads);
//   M T = L^-T W_sel with L read from scratch;  N V = Z_perm' T.
// A chain's result is a fixed function of its window and the settings: no atomics, nothing depends on the grid or on which workgroup ran it.
#include "lowrank_est_common.h"

namespace nphip_lrest_wide {

using namespace nphip_lrest_common;

struct Shape {
    static constexpr int R = 128;          // order of the subspace problem (2 x basis draws, zero-padded)
    static constexpr int LD = 130;         // column stride of the matrix in LDS (even: 16-byte accesses; 130 = 2 mod 32 spreads a row over the banks)
    static constexpr int kThreads = 1024;  // four waves per SIMD
    static constexpr int kMaxDim = 1024;
    static constexpr int kMaxPick = 64;
};
constexpr int R = Shape::R, LD = Shape::LD, kThreads = Shape::kThreads, kMaxDim = Shape::kMaxDim, kMaxPick = Shape::kMaxPick;
constexpr int kWaves = kThreads / 64;
constexpr int kDiag = 16;      // diagnostic words per chain
// per workgroup, in doubles: mean_x, mean_g, stds [kMaxDim each]; L, Cx, Cg -> Rc [R x R each]; the selected columns [R x kMaxK]
constexpr int kWgScratch = 3 * kMaxDim + 3 * R * R + R * kMaxK;
static_assert(kWgScratch == 54272, "include/nutpie_hip.h and nutpie_amd/_lib.py state this figure");
typedef nphip_lrest_common::Params<kMaxPick> Params;   // scratch: [grid][kWgScratch], then [n][kDiag]

// The thread index, made opaque to the compiler at the start of every phase: addresses derived from it are then computed where a phase
// uses them, not once ahead of the loop over chains — hoisted there they outlive every phase and the kernel spills (190 registers without this).
#define NPHIP_FRESH_TID() do { asm volatile("" : "+v"(tid)); ri = tid & 31; cj = tid >> 5; } while (0)

__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double t = red[tid & (kWaves - 1)];   // the 16 wave sums, added in one fixed butterfly by every thread
#pragma unroll
    for (int off = kWaves / 2; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// One-sided Jacobi (Hestenes) on the columns of F (R x R in LDS): on return the columns are mutually orthogonal, F_out = F_in J with J
// orthogonal — F F' is unchanged, column j is (eigenvector j of F F') x (eigenvalue j)^1/2.  J is not accumulated.  64 disjoint column
// pairs per step by the round-robin tournament (127 steps a sweep), 16 lanes per pair, 8 elements of each column per lane, one barrier
// per step, every operand read before the first dependent instruction.  Columns whose squared norm is below rel_tiny |F|_F^2 are zero.
__device__ int jacobi(double* __restrict__ F, double* __restrict__ red, int tid, double rel_tiny) {
    double fro = 0.0;
    for (int idx = tid; idx < R * R; idx += kThreads) { const double a = M_(F, idx & (R - 1), idx >> 7); fro = fma(a, a, fro); }
    fro = block_sum(fro, red, tid);
    const double tiny2 = fro * rel_tiny + 1e-300;
    const int pr = tid / kPairLanes, sub = tid % kPairLanes;
    int sweeps = 0;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        int rotated = 0;
        ++sweeps;
        for (int step = 0; step < R - 1; ++step) {
            int p, q;
            jacobi_pair<Shape>(pr, step, p, q);
            double* gp = F + p * LD + 2 * sub;
            double* gq = F + q * LD + 2 * sub;
            JacobiStep<Shape>::Col xp, xq;
            jacobi_load<Shape>(gp, gq, xp, xq);
            double a, b, g;
            jacobi_dots<Shape>(xp, xq, a, b, g);
            if (a > tiny2 && b > tiny2 && g * g > kJacobiTol2 * (a * b)) {   // |g| > tol sqrt(a b); columns below tiny2 are zero
                double c, s;
                jacobi_rotation(a, b, g, c, s);
                rotated = 1;
                jacobi_rotate_store<Shape>(gp, gq, xp, xq, c, s);
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) break;
    }
    return sweeps;
}

// out[j] = |column j|^2 restricted to rows [0, n) (8 threads per column)
__device__ void col_norm2(const double* __restrict__ F, double* __restrict__ out, int n, int tid) {
    const int j = tid >> 3, part = tid & 7;
    double acc = 0.0;
    for (int r = part * (R / 8); r < (part + 1) * (R / 8); ++r) { const double v = M_(F, r, j); acc = (r < n) ? fma(v, v, acc) : acc; }
    acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64);
    if (part == 0) out[j] = acc;
    __syncthreads();
}

// Cholesky factorisation in place, A = L L' (on return the lower triangle is L, the rest zero).  perm != nullptr: A symmetric with both
// triangles valid; diagonal pivoting and a rank decision — the factorisation of P A P' stops at the first pivot below rel_tol times the
// first (largest) one; perm[k] = the original index at position k; returns the rank (columns beyond it are zero).  perm == nullptr: plain
// Cholesky of a positive definite matrix, only the lower triangle is read.
__device__ int cholesky(double* __restrict__ A, int* __restrict__ perm, double rel_tol, double* __restrict__ red, int* __restrict__ ired, int tid) {
    if (perm && tid < R) perm[tid] = tid;
    __syncthreads();
    int rank = R;
    double d0 = 0.0;
    const int i = tid & (R - 1), tj = tid >> 7;
    for (int k = 0; k < R; ++k) {
        double dk;
        if (perm) {
            if (tid < 64) {   // wave 0, two diagonal entries per lane: the largest remaining one (ties: the lowest index)
                double da = (tid >= k) ? M_(A, tid, tid) : -__builtin_inf();
                double db = (tid + 64 >= k) ? M_(A, tid + 64, tid + 64) : -__builtin_inf();
                if (!(da == da)) da = -__builtin_inf();
                if (!(db == db)) db = -__builtin_inf();
                double best = fmax(da, db);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
                const unsigned long long ma = __ballot(da == best), mb = __ballot(db == best);
                if (tid == 0) { ired[0] = ma ? (__ffsll((long long)ma) - 1) : (__ffsll((long long)mb) - 1 + 64); red[0] = best; }
            }
            __syncthreads();
            const int piv = ired[0];
            dk = red[0];
            if (k == 0) d0 = dk;
            if (!(dk > rel_tol * d0) || !(dk > 0.0)) { rank = k; break; }
            if (piv != k) {
                if (tid < R) { const double t = M_(A, k, tid); M_(A, k, tid) = M_(A, piv, tid); M_(A, piv, tid) = t; }
                __syncthreads();
                if (tid < R) { const double t = M_(A, tid, k); M_(A, tid, k) = M_(A, tid, piv); M_(A, tid, piv) = t; }
                if (tid == 0) { const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t; }
            }
            __syncthreads();
        } else {
            dk = M_(A, k, k);
            if (!(dk > 0.0)) dk = 1e-300;   // (positive definite by construction: gamma on the diagonal)
            __syncthreads();
        }
        const double lkk = sqrt(dk), inv = 1.0 / lkk;
        if (tid > k && tid < R) M_(A, tid, k) *= inv;
        if (tid == k) M_(A, k, k) = lkk;
        __syncthreads();
        if (i > k) {   // thread (i, tj): row i of the columns k + 1 + tj, + 8, ...
            const double lik = M_(A, i, k);
            const int jend = perm ? R : i + 1;
            for (int j = k + 1 + tj; j < jend; j += kThreads / R) M_(A, i, j) = fma(-lik, M_(A, j, k), M_(A, i, j));
        }
        __syncthreads();
    }
    for (int idx = tid; idx < R * R; idx += kThreads) {
        const int ii = idx & (R - 1), j = idx >> 7;
        if (j > ii || j >= rank) M_(A, ii, j) = 0.0;
    }
    __syncthreads();
    return rank;
}

// B <- L^-T B in place: B the first nc columns of the LDS matrix, L lower triangular of order n (<= R) in device memory, ROW-major
// (Lrow[i * R + j] = L(i, j): row i is what step i reads).  Back substitution, right-looking; a thread has row tid & 127 of the columns
// tid >> 7, + 8, ...
__device__ void solve_lt(const double* __restrict__ Lrow, double* __restrict__ B, int n, int nc, int tid) {
    const int j = tid & (R - 1), cg = tid >> 7;
    for (int i = n - 1; i >= 0; --i) {
        const double inv = 1.0 / Lrow[i * R + i];
        if (tid < nc) M_(B, i, tid) *= inv;
        __syncthreads();
        if (j < i) {
            const double lij = Lrow[i * R + j];
            for (int c = cg; c < nc; c += kThreads / R) M_(B, j, c) = fma(-lij, M_(B, i, c), M_(B, j, c));
        }
        __syncthreads();
    }
}

// The spectrum of S (es: squared column norms; lv: the part of them inside the span) -> es re-centred, isel[0 .. n_used) the chosen
// directions, isel[kMaxK] = n_used; returns the centre.  Clamp to what a geometric mean of these two matrices can have, re-centre on the
// lower median of the directions inside the span, pick the k_max furthest from 1 (log scale) among those outside [1 / cutoff, cutoff];
// a thread per direction.  (A function of its own: inlined, the constants of its log and exp are set up ahead of the loop over chains
// and held in registers through every phase.)
__device__ __noinline__ double select(double* __restrict__ es, double* __restrict__ le, double* __restrict__ lv, double* __restrict__ red,
                                      int* __restrict__ isel, double trx, double trg, double gamma, double log_cutoff, int k_max, int tid) {
    if (tid < kMaxK + 4) isel[tid] = -1;
    if (tid < R) {
        // (bounds of the exact spectrum, from traces: |Cg| <= tr Cg, |Cx| <= tr Cx — a net for what rounding puts outside, not a rule)
        const double lo = sqrt(gamma / fmax(trg, gamma)), hi = sqrt(fmax(trx, gamma) / gamma);
        const double n2 = es[tid];
        const bool live = n2 > 0.0 && lv[tid] > 0.5 * n2;
        const double e = fmax(fmin(n2, hi), lo);
        es[tid] = e;
        le[tid] = log(e);
        lv[tid] = live ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < R) {
        const int j = tid;
        const bool live = lv[j] != 0.0;
        const double lj = le[j];
        int n_live = 0, below = 0;
        for (int i = 0; i < R; ++i) {
            const bool il = lv[i] != 0.0;
            const double li = le[i];
            n_live += il ? 1 : 0;
            below += (il && (li < lj || (li == lj && i < j))) ? 1 : 0;
        }
        if (live && below == (n_live - 1) / 2) red[17] = lj;   // the lower median (exactly one thread)
        if (j == 0 && n_live == 0) red[17] = 0.0;
    }
    __syncthreads();
    const double centre = exp(red[17]);
    if (tid < R) {
        const double e = es[tid] / centre;
        const double score0 = fabs(log(e));
        es[tid] = e;
        le[tid] = (lv[tid] != 0.0 && score0 > log_cutoff) ? score0 : -1.0;
    }
    __syncthreads();
    if (tid < R) {   // position in the descending order of the scores (ties: the lower index first)
        const int j = tid;
        const double sj = le[j];
        int before = 0, n_pos = 0;
        for (int i = 0; i < R; ++i) {
            const double si = le[i];
            n_pos += si > 0.0 ? 1 : 0;
            before += (si > sj || (si == sj && i < j)) ? 1 : 0;
        }
        if (sj > 0.0 && before < k_max) isel[before] = j;
        if (j == 0) isel[kMaxK] = n_pos < k_max ? n_pos : k_max;
    }
    __syncthreads();
    return centre;
}

__device__ void estimate_one(const Params& P, const int slot, double* lds) {
    double* A = lds;                     // the one R x R matrix
    double* es = A + R * LD;             // [R] spectrum
    double* le = es + R;                 // [R] its log, then the scores
    double* lv = le + R;                 // [R] squared norm of a direction inside the span
    double* red = lv + R;                // [24]: wave sums; [16] the pivot; [17] the spectrum's centre
    int* isel = (int*)(red + 24);        // [kMaxK + 4]
    int* perm = isel + kMaxK + 4;        // [R]
    const int* pick = perm + R;          // [kMaxPick]: P.pick, copied once per workgroup (a dynamic index into the kernel argument costs registers)
    int tid = threadIdx.x, ri, cj;
    NPHIP_FRESH_TID();
    double* gs = P.scratch + (size_t)blockIdx.x * kWgScratch;
    double* mean_x = gs;                 // [kMaxDim] each
    double* mean_g = mean_x + kMaxDim;
    double* stds = mean_g + kMaxDim;
    double* gL = stds + kMaxDim;         // L, row-major
    double* gCx = gL + R * R;            // Cx, column-major
    double* gCg = gCx + R * R;           // Cg, column-major; then Rc, row-major
    double* gT = gCg + R * R;            // the selected directions [kMaxK][R]
    double* dg = P.scratch + (size_t)gridDim.x * kWgScratch + (size_t)slot * kDiag;
    const long long chain = P.chains ? P.chains[slot] : (long long)slot;
    const double* X = P.draws + chain * P.chain_stride;
    const double* Gx = P.grads + chain * P.chain_stride;
    const int D = P.dim, m = P.m, b = P.b;
    const double inf = __builtin_inf();
    const long long tk0_ = (long long)__builtin_readcyclecounter();

    // ---- A. moments over the whole window (two passes) and the diagonal scaling sqrt(std(x) / std(g)); a thread has its own dimensions.
    //         lowrank_est_common.h: window_moments, written out — and so is phase N below (write_columns): called through the header, by
    //         value or through P, this kernel spills more registers at its ceiling of 128.  A change to either phase is made in both places.
    int bad = 0;
    for (int i = tid; i < D; i += kThreads) {
        double sx = 0.0, sg = 0.0;
        const double x0 = X[i], g0 = Gx[i];
        bool const_x = true, const_g = true;
        for (int t = 0; t < m; ++t) {
            const double x = X[(long long)t * P.draw_stride + i], g = Gx[(long long)t * P.draw_stride + i];
            if (!(fabs(x) < inf) || !(fabs(g) < inf)) bad = 1;
            const_x = const_x && x == x0; const_g = const_g && g == g0;
            sx += x; sg += g;
        }
        // (a coordinate that never moved has ITS value as mean, exactly)
        mean_x[i] = const_x ? x0 : sx / (double)m; mean_g[i] = const_g ? g0 : sg / (double)m;
    }
    bad = __syncthreads_or(bad);   // a window with a non-finite entry says nothing: the identity for this chain
    for (int i = tid; i < D; i += kThreads) {
        double st = 1.0;
        if (!bad) {
            const double mx = mean_x[i], mg = mean_g[i];
            double vx = 0.0, vg = 0.0;
            for (int t = 0; t < m; ++t) {
                const double dx = X[(long long)t * P.draw_stride + i] - mx, dg_ = Gx[(long long)t * P.draw_stride + i] - mg;
                vx = fma(dx, dx, vx); vg = fma(dg_, dg_, vg);
            }
            const double sdx = sqrt(vx / (double)(m - 1)), sdg = sqrt(vg / (double)(m - 1));
            st = sqrt(sdx / sdg);
            if (!(fabs(st) < inf) || !(st > 0.0)) st = 1.0;
            st = fmin(fmax(st, 1e-10), 1e10);
        } else {
            mean_x[i] = 0.0; mean_g[i] = 0.0;
        }
        stds[i] = st;
    }
    __syncthreads();   // (also makes the scratch writes visible to the workgroup)

    const BasisRows zval{X, Gx, pick, P.draw_stride, mean_x, mean_g, stds, b, bad};

    // a thread's 4 x 4 block of an R x R product: rows ri + 32 i', columns cj + 32 j' (interleaved: the reads along a row of the matrix
    // then fall on 16 bank pairs, and cj is uniform over half a wave): ri = tid & 31, cj = tid >> 5

    NPHIP_FRESH_TID();
    // ---- B. Gram matrix G = Z Z': tiles of 32 dimensions staged in the matrix area (columns 0 .. 31), accumulators in registers
    {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int d0 = 0; d0 < D; d0 += 32) {
            __syncthreads();
            for (int e = tid; e < R * 32; e += kThreads) {
                const int dl = e & 31, t = e >> 5;
                M_(A, t, dl) = (d0 + dl < D) ? zval(t, d0 + dl) : 0.0;
            }
            __syncthreads();
            for (int k = 0; k < 32; ++k) {
                double a[4], bb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = M_(A, ri + 32 * i, k);
#pragma unroll
                for (int j = 0; j < 4; ++j) bb[j] = M_(A, cj + 32 * j, k);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], bb[j], acc[i][j]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) M_(A, ri + 32 * i, cj + 32 * j) = acc[i][j];
        __syncthreads();
    }

    NPHIP_FRESH_TID();
    // ---- C. the basis rows in an orthonormal basis of their span: Z_perm = L Q' from the pivoted Cholesky factorisation of the Gram
    //         matrix (rank: pivots above 1e-10 of the first).  L is parked for the end (V = Q W_sel = Z_perm' L^-T W_sel).
    const long long t0_ = (long long)__builtin_readcyclecounter();
    const int rank = cholesky(A, perm, 1e-10, red + 16, isel, tid);
    for (int idx = tid; idx < R * R; idx += kThreads) gL[idx] = M_(A, idx >> 7, idx & (R - 1));   // gL[k * R + i] = L(k, i)

    NPHIP_FRESH_TID();
    // ---- E. Cx = Px' Px / b + gamma I, Cg = Pg' Pg / b + gamma I: row k of L is a draw (perm[k] < b) or a gradient
    int nonfin = 0;
    double trx = 0.0, trg = 0.0;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {   // (Cx, then Cg: one 4 x 4 block of accumulators at a time keeps the kernel inside 128 registers)
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int k = 0; k < R; ++k) {   // (every position: with a rank below r a basis row can sit anywhere; the rows of the zero padding are zero)
            if ((perm[k] < b) != (which == 0)) continue;
            double a[4], bb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = M_(A, k, ri + 32 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) bb[j] = M_(A, k, cj + 32 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * bb[j];
        }
        double* const out = which == 0 ? gCx : gCg;
        double tr = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rr = ri + 32 * i, c = cj + 32 * j;
                const double v = acc[i][j] / (double)b + ((rr == c) ? P.gamma : 0.0);
                out[c * R + rr] = v;
                if (!(fabs(v) < inf)) nonfin = 1;
                if (rr == c && rr < rank) tr += v;
            }
        if (which == 0) trx = tr; else trg = tr;
    }
    nonfin = __syncthreads_or(nonfin);   // a Gram matrix that overflowed says as little as a non-finite window
    trx = block_sum(trx, red, tid);
    trg = block_sum(trg, red, tid);
    if (bad || nonfin) {
        write_identity<Shape>(P, slot, tid);
        if (tid < kDiag) dg[tid] = 0.0;
        return;
    }

    NPHIP_FRESH_TID();
    // ---- F. Cg = Rc Rc' (Cholesky), Rc parked row-major; Cx = Lx Lx'; F1 = Rc' Lx in registers, then over the matrix
    const long long t1_ = (long long)__builtin_readcyclecounter();
    for (int idx = tid; idx < R * R; idx += kThreads) M_(A, idx & (R - 1), idx >> 7) = gCg[idx];
    __syncthreads();
    cholesky(A, nullptr, 0.0, red + 16, isel, tid);
    for (int idx = tid; idx < R * R; idx += kThreads) gCg[idx] = M_(A, idx >> 7, idx & (R - 1));   // gCg[k * R + i] = Rc(k, i)
    __syncthreads();
    NPHIP_FRESH_TID();
    for (int idx = tid; idx < R * R; idx += kThreads) M_(A, idx & (R - 1), idx >> 7) = gCx[idx];
    __syncthreads();
    cholesky(A, nullptr, 0.0, red + 16, isel, tid);
    NPHIP_FRESH_TID();
    {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int k = 0; k < R; ++k) {   // F1(i, j) = sum_k Rc(k, i) Lx(k, j)
            double a[4], bb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = gCg[k * R + ri + 32 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bb[j] = M_(A, k, cj + 32 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], bb[j], acc[i][j]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) M_(A, ri + 32 * i, cj + 32 * j) = acc[i][j];
        __syncthreads();
    }

    NPHIP_FRESH_TID();
    // ---- H. columns of F1 -> u_j s_j;  I. scaled by s_j^-1/2 (s_j^2 is the column's squared norm), then F2 = Rc^-T (U S^1/2)
    const long long t2_ = (long long)__builtin_readcyclecounter();
    const int sw1 = jacobi(A, red, tid, 1e-40);
    col_norm2(A, es, R, tid);
    for (int idx = tid; idx < R * R; idx += kThreads) {
        const int c = idx >> 7;
        const double s2 = es[c];
        M_(A, idx & (R - 1), c) *= (s2 > 0.0) ? sqrt(sqrt(1.0 / s2)) : 0.0;
    }
    __syncthreads();
    NPHIP_FRESH_TID();
    const long long t3_ = (long long)__builtin_readcyclecounter();
    solve_lt(gCg, A, R, R, tid);
    NPHIP_FRESH_TID();
    // ---- J. columns of F2 -> w_j e_j^1/2: the spectrum of S and its eigenvectors, already in the coordinates of Q
    const long long t4_ = (long long)__builtin_readcyclecounter();
    const int sw2 = jacobi(A, red, tid, 1e-40);
    const long long t5_ = (long long)__builtin_readcyclecounter();
    col_norm2(A, es, R, tid);
    col_norm2(A, lv, rank, tid);

    NPHIP_FRESH_TID();
    // ---- L. spectrum: clamped, re-centred, the k_max directions chosen (select)
    const double centre = select(es, le, lv, red, isel, trx, trg, P.gamma, P.log_cutoff, P.k_max, tid);
    const int n_used = isel[kMaxK];
    write_spectrum<Shape>(P, slot, stds, centre, es, isel, n_used, tid);

    NPHIP_FRESH_TID();
    // ---- M. T = L^-T W[:, sel]  (rank x n_used; rows beyond the rank are zero): the selected columns, normalised, go through the scratch
    //         to columns 0 .. 15 of the matrix area; L is read from the scratch.  N. V = Q W_sel = Z_perm' T
    for (int idx = tid; idx < R * kMaxK; idx += kThreads) {
        const int i = idx & (R - 1), jj = idx >> 7;
        double v = 0.0;
        if (jj < n_used && i < rank) {
            const int c = isel[jj];
            double n2 = 0.0;   // (the column's squared norm, summed in one fixed order by every thread that needs it)
            for (int q = 0; q < R; ++q) { const double w = M_(A, q, c); n2 = fma(w, w, n2); }
            v = M_(A, i, c) * fast_rsq(n2);
        }
        gT[idx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < R * kMaxK; idx += kThreads) M_(A, idx & (R - 1), idx >> 7) = gT[idx];
    __syncthreads();
    NPHIP_FRESH_TID();
    solve_lt(gL, A, rank, kMaxK, tid);
    NPHIP_FRESH_TID();
    // (N: lowrank_est_common.h: write_columns, kept here — see phase A)
    for (int i = tid; i < D; i += kThreads) {
        double acc[kMaxK];
#pragma unroll
        for (int jj = 0; jj < kMaxK; ++jj) acc[jj] = 0.0;
        if (n_used > 0) {
            for (int t = 0; t < rank; ++t) {
                const double z = zval(perm[t], i);
#pragma unroll
                for (int jj = 0; jj < kMaxK; ++jj) acc[jj] = fma(z, M_(A, t, jj), acc[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < kMaxK; ++jj)
            if (jj < P.k_max) P.V[((size_t)slot * P.k_max + jj) * D + i] = (jj < n_used) ? acc[jj] : 0.0;
    }
    if (tid == 0) {   // diagnostics: sweeps of the two solvers, then cycles (moments + Gram, pivoted Cholesky + Cx/Cg, the two factors + F1,
                      // first Jacobi pass, back substitution, second Jacobi pass, everything)
        const long long t6_ = (long long)__builtin_readcyclecounter();
        dg[0] = sw1; dg[1] = sw2; dg[2] = rank;
        dg[3] = (double)(t0_ - tk0_); dg[4] = (double)(t1_ - t0_); dg[5] = (double)(t2_ - t1_); dg[6] = (double)(t3_ - t2_);
        dg[7] = (double)(t4_ - t3_); dg[8] = (double)(t5_ - t4_); dg[9] = (double)(t6_ - tk0_);
        for (int w = 10; w < kDiag; ++w) dg[w] = 0.0;
    }
}

// A workgroup takes the chains slot, slot + gridDim.x, ... through its LDS and its block of the scratch (the launch is capped at the CUs
// the running engine kernel leaves idle: a workgroup's 137 KB of LDS want a CU to themselves)
__global__ __launch_bounds__(kThreads) void k_lr_estimate_wide(const Params P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    {
        int* pick = (int*)(lds + R * LD + 3 * R + 24) + kMaxK + 4 + R;
        if (threadIdx.x < kMaxPick) pick[threadIdx.x] = P.pick[threadIdx.x];
        __syncthreads();
    }
    for (int slot = blockIdx.x; slot < P.n; slot += gridDim.x) {
        estimate_one(P, slot, lds);
        __syncthreads();
    }
}

constexpr size_t kLdsBytes = ((size_t)R * LD + 3 * R + 24) * sizeof(double) + (kMaxK + 4 + R + kMaxPick) * sizeof(int) + 16;

}  // namespace nphip_lrest_wide

extern "C" int nphip_low_rank_estimate_wide_supported(uint64_t dim, uint64_t m, uint64_t n_pick, uint64_t k_max) {
    return nphip_lrest_common::shape_supported<nphip_lrest_wide::Shape>(dim, m, n_pick, k_max) ? 1 : 0;
}

extern "C" int nphip_low_rank_estimate_wide(uint64_t n, uint64_t dim, uint64_t m, uint64_t n_pick, const int32_t* pick, const double* draws, const double* grads,
                                            int64_t chain_stride, int64_t draw_stride, const int64_t* chains_device, double gamma, double cutoff, uint64_t k_max,
                                            double* sigma2, double* V, double* lambda, int32_t* k_used, double* scratch, uint64_t max_workgroups, void* stream) {
    using namespace nphip_lrest_wide;
    return nphip_lrest_common::launch<Shape>(k_lr_estimate_wide, kLdsBytes, n, dim, m, n_pick, pick, draws, grads, chain_stride, draw_stride, chains_device, gamma, cutoff,
                                             k_max, sigma2, V, lambda, k_used, scratch, max_workgroups, stream);
}
