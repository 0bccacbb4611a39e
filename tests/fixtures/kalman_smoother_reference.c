/* The order contract of the Kalman smoother stage, restated as plain loops: what tests/test_gpu_kalman_smoother_stages.py
 * holds nutpie_amd/csrc/kalman_smoother.h to, bit for bit.  Built by tests/kalman_smoother_reference.py with -ffp-contract=off: every
 * fused multiply-add is written as fma(), every other operation is one IEEE operation in the order written, every division a true one.
 * This file is the normative text of the contract.
 *
 * R series of T steps, state dimension m <= 8.  obs: R x T (read only when `masked`; 0: a missing step); Z: R x T x m; Tm: m x m
 * row-major, shared by the series, not read when T = 1.
 * F = [apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T]: what the filter stored (tests/fixtures/kalman_reference.c);
 *     afilt is not read.
 * S = [asm: R T m | vsm: R T m]: the smoothed mean of the state, and the diagonal of its smoothed covariance. */
#include <math.h>

#define MS 8

/* dot_k: s = +0.0, then s = fma(x_k, y_k, s) for ascending k; sx / sy the strides */
static double dotk(const double* x, int sx, const double* y, int sy, int m) {
    double s = 0.0;
    for (int k = 0; k < m; ++k) s = fma(x[k * sx], y[k * sy], s);
    return s;
}

void kalman_smooth(int R, int T, int m, int masked, const double* obs, const double* Z, const double* Tm, const double* F, double* S) {
    const double* apred = F;
    const double* Ppred = apred + (long)R * T * m;
    const double* vs = Ppred + (long)R * T * m * m + (long)R * T * m;
    const double* Fs = vs + (long)R * T;
    double* mean = S;
    double* var = mean + (long)R * T * m;
    double r[MS], N[MS * MS], u[MS], V[MS * MS], W[MS * MS], K[MS], g[MS], gt[MS], Y[MS * MS];
    for (int q = 0; q < R; ++q) {
        for (int i = 0; i < m; ++i) r[i] = 0.0;
        for (int i = 0; i < m * m; ++i) N[i] = 0.0;
        for (int t = T - 1; t >= 0; --t) {
            const long s = (long)q * T + t;
            const double* z = Z + s * m;
            const double* a = apred + s * m;
            const double* P = Ppred + s * m * m;
            const int seen = !masked || obs[s] != 0.0;
            const double v = vs[s], Fv = Fs[s];
            if (t < T - 1) {
                for (int k = 0; k < m; ++k) u[k] = dotk(Tm + k, m, r, 1, m);
                for (int k = 0; k < m; ++k)
                    for (int j = 0; j < m; ++j) V[k * m + j] = dotk(Tm + k, m, N + j, m, m);
                for (int k = 0; k < m; ++k)
                    for (int l = 0; l < m; ++l) W[k * m + l] = dotk(V + k * m, 1, Tm + l, m, m);
            } else {
                for (int i = 0; i < m; ++i) u[i] = 0.0;
                for (int i = 0; i < m * m; ++i) W[i] = 0.0;
            }
            if (seen) {
                for (int i = 0; i < m; ++i) K[i] = dotk(P + i * m, 1, z, 1, m) / Fv;
                const double e = v / Fv - dotk(K, 1, u, 1, m);
                for (int i = 0; i < m; ++i) g[i] = dotk(W + i * m, 1, K, 1, m);
                for (int j = 0; j < m; ++j) gt[j] = dotk(W + j, m, K, 1, m);
                const double D = 1.0 / Fv + dotk(K, 1, g, 1, m);
                for (int k = 0; k < m; ++k) r[k] = fma(e, z[k], u[k]);
                for (int i = 0; i < m; ++i) {
                    const double Dz = D * z[i];
                    for (int j = 0; j < m; ++j) N[i * m + j] = fma(Dz, z[j], fma(-g[i], z[j], fma(-z[i], gt[j], W[i * m + j])));
                }
            } else {
                for (int i = 0; i < m; ++i) r[i] = u[i];
                for (int i = 0; i < m * m; ++i) N[i] = W[i];
            }
            for (int i = 0; i < m; ++i) mean[s * m + i] = a[i] + dotk(P + i * m, 1, r, 1, m);
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) Y[i * m + j] = dotk(P + i * m, 1, N + j, m, m);
            for (int i = 0; i < m; ++i) var[s * m + i] = P[i * m + i] - dotk(Y + i * m, 1, P + i * m, 1, m);
        }
    }
}
