// nutpie-hip: what the two window-estimator kernels of adaptation="low_rank" share — lowrank_est.hip (subspace of order 64) and
// lowrank_est_wide.hip (order 128).  Only code that is the same in both is here, as forceinline functions over a shape struct S
// (S::R, S::LD, S::kThreads, S::kMaxDim, S::kMaxPick); nothing here asks which kernel is calling.  Where the kernels differ in arithmetic
// order or loop shape each keeps its own code: the block sums (their summation orders differ), the Cholesky factorisations, the back
// substitutions, the matrix products, the selection of directions and the Jacobi driver loops (the narrow one accumulates eigenvectors).
//
// The contract both kernels keep: moments over all m draws of the window, a constant coordinate is its own mean, a non-finite window or
// an overflowed Gram matrix is exactly the identity, rank at 1e-10 of the first Cholesky pivot, spectrum clamped to the trace bounds,
// re-centred on the lower median over the live directions, the k_max directions by |log| outside the cutoff with ties to the lower index;
// a chain's result is a fixed function of its window and the settings — nothing depends on the grid or on which workgroup ran it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/nutpie_hip.h"

namespace nphip_lrest_common {

constexpr int kMaxK = 16;
constexpr int kMaxSweeps = 30;
constexpr double kJacobiTol2 = 1e-28;   // a pair of columns is orthogonal when |g_p . g_q| <= 1e-14 |g_p| |g_q|
constexpr int kPairLanes = 16;          // lanes per column pair of a Jacobi step: one DPP row

template <int MAXPICK>
struct Params {
    const double* draws;
    const double* grads;
    long long chain_stride, draw_stride;
    const long long* chains;   // device, or null: chain = slot
    int n, dim, m, b;
    int pick[MAXPICK];
    double gamma, log_cutoff;
    int k_max;
    double* sig2;     // [n][dim]
    double* V;        // [n][k_max][dim]
    double* lam;      // [n][k_max]
    int* k_used;      // [n]
    double* scratch;  // (layout: the kernel's own)
};

// element (r, c) of a matrix in LDS: column-major with the column stride LD of the scope it is used in
#define M_(A, r, c) (A)[(c) * LD + (r)]

// 1 / sqrt(x) and 1 / x to full precision from the hardware's seeds (two / one Newton steps more than the seed's ~26 bits need: the
// compiler's own sqrt and divide carry scaling for denormals and a correctly rounded last bit this rotation has no use for — its angle
// may be off in the last bits as long as c^2 + s^2 = 1, which the refined rsq gives)
__device__ __forceinline__ double fast_rsq(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double hx = 0.5 * x;
    y = fma(y, fma(-hx * y, y, 0.5), y);
    y = fma(y, fma(-hx * y, y, 0.5), y);
    return y;
}
__device__ __forceinline__ double fast_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(y, fma(-x, y, 1.0), y);
    y = fma(y, fma(-x, y, 1.0), y);
    return y;
}

// sum over the 16 lanes that share a column pair, returned to all of them.  16 lanes are one DPP row: four v_mov_dpp steps (quad
// permutations, then the half-row and row mirrors — after each step the partial sums are uniform over the group the next one crosses),
// no trip through the LDS crossbar (ds_bpermute: what __shfl_xor compiles to — ~100 cycles of latency per level, twelve levels in a chain)
template <int CTRL> __device__ __forceinline__ double dpp_get(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void pair_sum3(double& a, double& b, double& g) {
    a += dpp_get<0xB1>(a); b += dpp_get<0xB1>(b); g += dpp_get<0xB1>(g);
    a += dpp_get<0x4E>(a); b += dpp_get<0x4E>(b); g += dpp_get<0x4E>(g);
    a += dpp_get<0x141>(a); b += dpp_get<0x141>(b); g += dpp_get<0x141>(g);
    a += dpp_get<0x140>(a); b += dpp_get<0x140>(b); g += dpp_get<0x140>(g);
}

// ---- one step of the one-sided Jacobi method (Hestenes) on the columns of an R x R matrix in LDS: R / 2 disjoint column pairs rotate in
// parallel, 16 lanes per pair, each lane with NJ 16-byte pieces of both columns.  The driver loops (sweeps, steps, the barrier per step,
// what else is rotated along) are the kernels' own.
template <class S> struct JacobiStep {
    static constexpr int NJ = (S::R / kPairLanes) / 2;   // 16-byte pieces of a column per lane
    typedef double2 Col[NJ];
};

// the columns (p, q) that pair `pr` of 0 .. R / 2 - 1 rotates at `step` of 0 .. R - 2: the round-robin tournament
template <class S> __device__ __forceinline__ void jacobi_pair(int pr, int step, int& p, int& q) {
    constexpr int R = S::R;
    if (pr == 0) { p = R - 1; q = step; }
    else { p = step + pr; p -= (p >= R - 1) ? R - 1 : 0; q = step + (R - 1) - pr; q -= (q >= R - 1) ? R - 1 : 0; }
}

// this lane's pieces of the columns at cp, cq (the column's address plus 2 x the lane's index in its group of 16)
template <class S> __device__ __forceinline__ void jacobi_load(const double* cp, const double* cq, typename JacobiStep<S>::Col& xp, typename JacobiStep<S>::Col& xq) {
#pragma unroll
    for (int j = 0; j < JacobiStep<S>::NJ; ++j) { xp[j] = *(const double2*)(cp + 2 * kPairLanes * j); xq[j] = *(const double2*)(cq + 2 * kPairLanes * j); }
}

// a = |x_p|^2, b = |x_q|^2, g = x_p . x_q over the whole columns, in every lane of the pair
template <class S> __device__ __forceinline__ void jacobi_dots(const typename JacobiStep<S>::Col& xp, const typename JacobiStep<S>::Col& xq, double& a, double& b, double& g) {
    a = 0.0; b = 0.0; g = 0.0;
#pragma unroll
    for (int j = 0; j < JacobiStep<S>::NJ; ++j) {
        a = fma(xp[j].x, xp[j].x, a); a = fma(xp[j].y, xp[j].y, a);
        b = fma(xq[j].x, xq[j].x, b); b = fma(xq[j].y, xq[j].y, b);
        g = fma(xp[j].x, xq[j].x, g); g = fma(xp[j].y, xq[j].y, g);
    }
    pair_sum3(a, b, g);
}

// the rotation that makes the columns of a pair orthogonal:  tan of the angle t = sign(d) 2g / (|d| + sqrt(d^2 + 4 g^2)), d = b - a;
// c = 1 / sqrt(1 + t^2), s = c t.  (Whether a pair is rotated at all is tested in the driver loops, inline: behind a function of its own
// the same test compiles to other code around it — the narrow kernel then spills four more registers.)
__device__ __forceinline__ void jacobi_rotation(double a, double b, double g, double& c, double& s) {
    const double d = b - a, g2 = 2.0 * g;
    const double h2 = fma(d, d, g2 * g2);
    const double h = h2 * fast_rsq(h2);
    const double t = copysign(g2, d * g2) * fast_rcp(fabs(d) + h);
    c = fast_rsq(fma(t, t, 1.0));
    s = c * t;
}

// (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q), stored over the columns at cp, cq
template <class S> __device__ __forceinline__ void jacobi_rotate_store(double* cp, double* cq, const typename JacobiStep<S>::Col& xp, const typename JacobiStep<S>::Col& xq, double c, double s) {
#pragma unroll
    for (int j = 0; j < JacobiStep<S>::NJ; ++j) {
        double2 u, v;
        u.x = fma(c, xp[j].x, -(s * xq[j].x)); u.y = fma(c, xp[j].y, -(s * xq[j].y));
        v.x = fma(s, xp[j].x, c * xq[j].x);    v.y = fma(s, xp[j].y, c * xq[j].y);
        *(double2*)(cp + 2 * kPairLanes * j) = u; *(double2*)(cq + 2 * kPairLanes * j) = v;
    }
}

// ---- A. moments over the whole window (two passes, as torch.mean / torch.std do) and the diagonal scaling sqrt(std(x) / std(g)),
// clamped to [1e-10, 1e10]; a thread has its own dimensions.  mean_x, mean_g, stds: [dim] each, in LDS or in device memory (the barrier
// at the end makes either visible to the workgroup).  Returns whether the window has a non-finite entry: such a window says nothing —
// the means are then zero, the scaling one, and the caller writes the identity for this chain.
template <class S, class PT>
__device__ __forceinline__ int window_moments(const PT& P, const double* X, const double* Gx, double* mean_x, double* mean_g, double* stds, int tid) {
    const int D = P.dim, m = P.m;
    const double inf = __builtin_inf();
    int bad = 0;
    for (int i = tid; i < D; i += S::kThreads) {
        double sx = 0.0, sg = 0.0;
        const double x0 = X[i], g0 = Gx[i];
        bool const_x = true, const_g = true;
        for (int t = 0; t < m; ++t) {
            const double x = X[(long long)t * P.draw_stride + i], g = Gx[(long long)t * P.draw_stride + i];
            if (!(fabs(x) < inf) || !(fabs(g) < inf)) bad = 1;
            const_x = const_x && x == x0; const_g = const_g && g == g0;
            sx += x; sg += g;
        }
        // a coordinate that never moved (a chain whose proposals were all rejected) has ITS value as mean, exactly: the rounded sum over m
        // misses it by an ulp, and the ratio of two such residues came out as the scaling (sigma^2 = 32, 256, ... for a constant window)
        mean_x[i] = const_x ? x0 : sx / (double)m; mean_g[i] = const_g ? g0 : sg / (double)m;
    }
    bad = __syncthreads_or(bad);
    for (int i = tid; i < D; i += S::kThreads) {
        double st = 1.0;
        if (!bad) {
            const double mx = mean_x[i], mg = mean_g[i];
            double vx = 0.0, vg = 0.0;
            for (int t = 0; t < m; ++t) {
                const double dx = X[(long long)t * P.draw_stride + i] - mx, dg = Gx[(long long)t * P.draw_stride + i] - mg;
                vx = fma(dx, dx, vx); vg = fma(dg, dg, vg);
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
    __syncthreads();
    return bad;
}

// Z(t, i): row t of the scaled basis — draws for t < b, gradients for b <= t < 2b, zero padding beyond; all zero for a bad window.
// Never materialised: rebuilt from the trace where it is needed (the Gram matrix, and V at the end).
struct BasisRows {
    const double* X;
    const double* Gx;
    const int* pick;
    long long draw_stride;
    const double* mean_x;
    const double* mean_g;
    const double* stds;
    int b, bad;
    __device__ __forceinline__ double operator()(int t, int i) const {
        if (bad || t >= 2 * b) return 0.0;
        if (t < b) return (X[(long long)pick[t] * draw_stride + i] - mean_x[i]) / stds[i];
        return (Gx[(long long)pick[t - b] * draw_stride + i] - mean_g[i]) * stds[i];
    }
};

// the metric of a window that says nothing (a non-finite entry, an overflowed Gram matrix): exactly the identity, no column
template <class S, class PT> __device__ __forceinline__ void write_identity(const PT& P, int slot, int tid) {
    const int D = P.dim;
    for (int i = tid; i < D; i += S::kThreads) P.sig2[(size_t)slot * D + i] = 1.0;
    for (int idx = tid; idx < P.k_max * D; idx += S::kThreads) P.V[(size_t)slot * P.k_max * D + idx] = 0.0;
    if (tid < P.k_max) P.lam[(size_t)slot * P.k_max + tid] = 1.0;
    if (tid == 0) P.k_used[slot] = 0;
}

// sigma^2 (the scaling times the spectrum's centre), lambda (es: the re-centred spectrum; isel[0 .. n_used): the chosen directions) and
// the number of columns
template <class S, class PT>
__device__ __forceinline__ void write_spectrum(const PT& P, int slot, const double* stds, double centre, const double* es, const int* isel, int n_used, int tid) {
    const int D = P.dim;
    for (int i = tid; i < D; i += S::kThreads) { const double s = stds[i] * sqrt(centre); P.sig2[(size_t)slot * D + i] = s * s; }
    if (tid < P.k_max) P.lam[(size_t)slot * P.k_max + tid] = (tid < n_used) ? es[isel[tid]] : 1.0;
    if (tid == 0) P.k_used[slot] = n_used;
}

// ---- N. V = Q W_sel = Z_perm' T: T (rank x kMaxK, columns beyond n_used zero) in the first columns of the LDS matrix, a thread has its
// own dimensions
template <class S, class PT, class Z>
__device__ __forceinline__ void write_columns(const PT& P, int slot, const double* T, const int* perm, int rank, int n_used, const Z& zval, int tid) {
    constexpr int LD = S::LD;
    const int D = P.dim;
    for (int i = tid; i < D; i += S::kThreads) {
        double acc[kMaxK];
#pragma unroll
        for (int jj = 0; jj < kMaxK; ++jj) acc[jj] = 0.0;
        if (n_used > 0) {
            for (int t = 0; t < rank; ++t) {
                const double z = zval(perm[t], i);
#pragma unroll
                for (int jj = 0; jj < kMaxK; ++jj) acc[jj] = fma(z, M_(T, t, jj), acc[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < kMaxK; ++jj)
            if (jj < P.k_max) P.V[((size_t)slot * P.k_max + jj) * D + i] = (jj < n_used) ? acc[jj] : 0.0;
    }
}

// ---- host side
template <class S> inline bool shape_supported(uint64_t dim, uint64_t m, uint64_t n_pick, uint64_t k_max) {
    return dim >= 1 && dim <= (uint64_t)S::kMaxDim && m >= 2 && n_pick >= 1 && n_pick <= (uint64_t)S::kMaxPick && n_pick <= m && n_pick <= dim &&
           k_max >= 1 && k_max <= (uint64_t)kMaxK;
}

// Validates, fills Params, raises the kernel's dynamic LDS limit and launches: a workgroup takes the chains slot, slot + grid, ...; the
// grid is capped at max_workgroups (the CUs a running engine kernel leaves idle).
template <class S>
inline int launch(void (*kernel)(const Params<S::kMaxPick>), size_t lds_bytes, uint64_t n, uint64_t dim, uint64_t m, uint64_t n_pick, const int32_t* pick,
                  const double* draws, const double* grads, int64_t chain_stride, int64_t draw_stride, const int64_t* chains_device, double gamma, double cutoff,
                  uint64_t k_max, double* sigma2, double* V, double* lambda, int32_t* k_used, double* scratch, uint64_t max_workgroups, void* stream) {
    if (n == 0) return NPHIP_OK;
    if (!shape_supported<S>(dim, m, n_pick, k_max) || !pick || !draws || !grads || !sigma2 || !V || !lambda || !k_used || !scratch || !(cutoff > 1.0) || !(gamma > 0.0))
        return NPHIP_ERR;
    Params<S::kMaxPick> P;
    P.draws = draws; P.grads = grads; P.chain_stride = chain_stride; P.draw_stride = draw_stride; P.chains = (const long long*)chains_device;
    P.n = (int)n; P.dim = (int)dim; P.m = (int)m; P.b = (int)n_pick;
    for (int i = 0; i < S::kMaxPick; ++i) P.pick[i] = i < (int)n_pick ? pick[i] : 0;
    for (int i = 0; i < (int)n_pick; ++i) if (pick[i] < 0 || (uint64_t)pick[i] >= m) return NPHIP_ERR;
    P.gamma = gamma; P.log_cutoff = log(cutoff); P.k_max = (int)k_max;
    P.sig2 = sigma2; P.V = V; P.lam = lambda; P.k_used = k_used; P.scratch = scratch;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return NPHIP_ERR;
    const uint64_t grid = (max_workgroups > 0 && max_workgroups < n) ? max_workgroups : n;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(S::kThreads), lds_bytes, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? NPHIP_OK : NPHIP_ERR;
}

}  // namespace nphip_lrest_common
