/* The order contract of the Kalman filter stages, restated as plain loops: what tests/test_gpu_kalman_stages.py
 * holds nutpie_amd/csrc/chain_kalman.h to, bit for bit.  Built by tests/kalman_reference.py with -ffp-contract=off: every fused
 * multiply-add is written as fma(), every other operation is one IEEE operation in the order written, every division a true one.
 * This file is the normative text of the contract.
 *
 * R series of T steps, state dimension m <= 8.  y, h, obs: R x T; Z: R x T x m; Tm, Q, P0: m x m row-major; a0: m; all series share
 * Tm, Q, a0, P0.  obs is read only when `masked` (0: a missing step).
 * F = [apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T]
 * B = [ybar: R T | hbar: R T | Zbar: R T m | Tbar: m m | Qbar: m m | a0bar: m | P0bar: m m | partials: R x (Tb: m m | Qb: m m | a0b: m | P0b: m m)] */
#include <math.h>

#define MS 8

/* dot_k: s = +0.0, then s = fma(x_k, y_k, s) for ascending k; sx / sy the strides */
static double dotk(const double* x, int sx, const double* y, int sy, int m) {
    double s = 0.0;
    for (int k = 0; k < m; ++k) s = fma(x[k * sx], y[k * sy], s);
    return s;
}

/* the measurement update of one step from the predicted a, P: M, K, af, Pf (v and Fv are given) */
static void update(int m, int seen, const double* a, const double* P, const double* Z, double v, double Fv, double* M, double* K, double* af,
                   double* Pf) {
    if (seen) {
        for (int i = 0; i < m; ++i) M[i] = dotk(P + i * m, 1, Z, 1, m);
        for (int i = 0; i < m; ++i) K[i] = M[i] / Fv;
        for (int i = 0; i < m; ++i) af[i] = fma(K[i], v, a[i]);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) Pf[i * m + j] = fma(-K[i], M[j], P[i * m + j]);
    } else {
        for (int i = 0; i < m; ++i) af[i] = a[i];
        for (int i = 0; i < m * m; ++i) Pf[i] = P[i];
    }
}

void kalman_forward(int R, int T, int m, int masked, const double* y, const double* obs, const double* Z, const double* h, const double* Tm,
                    const double* Q, const double* a0, const double* P0, double* F) {
    double* apred = F;
    double* Ppred = apred + (long)R * T * m;
    double* afilt = Ppred + (long)R * T * m * m;
    double* vs = afilt + (long)R * T * m;
    double* Fs = vs + (long)R * T;
    double a[MS], P[MS * MS], M[MS], K[MS], af[MS], Pf[MS * MS], X[MS * MS];
    for (int r = 0; r < R; ++r) {
        for (int i = 0; i < m; ++i) a[i] = a0[i];
        for (int i = 0; i < m * m; ++i) P[i] = P0[i];
        for (int t = 0; t < T; ++t) {
            const long s = (long)r * T + t;
            const double* z = Z + s * m;
            const int seen = !masked || obs[s] != 0.0;
            for (int i = 0; i < m; ++i) apred[s * m + i] = a[i];
            for (int i = 0; i < m * m; ++i) Ppred[s * m * m + i] = P[i];
            double v = 0.0, Fv = 1.0;
            if (seen) {
                v = y[s] - dotk(z, 1, a, 1, m);
                for (int i = 0; i < m; ++i) M[i] = dotk(P + i * m, 1, z, 1, m);
                Fv = h[s] + dotk(z, 1, M, 1, m);
            }
            update(m, seen, a, P, z, v, Fv, M, K, af, Pf);
            vs[s] = v;
            Fs[s] = Fv;
            for (int i = 0; i < m; ++i) afilt[s * m + i] = af[i];
            if (t < T - 1) {
                for (int i = 0; i < m; ++i) a[i] = dotk(Tm + i * m, 1, af, 1, m);
                for (int i = 0; i < m; ++i)
                    for (int j = 0; j < m; ++j) X[i * m + j] = dotk(Pf + i * m, 1, Tm + j * m, 1, m);
                for (int i = 0; i < m; ++i)
                    for (int j = 0; j < m; ++j) P[i * m + j] = Q[i * m + j] + dotk(Tm + i * m, 1, X + j, m, m);
            }
        }
    }
}

void kalman_backward(int R, int T, int m, int masked, const double* y, const double* obs, const double* Z, const double* h, const double* Tm,
                     const double* Q, const double* F, const double* vbar, const double* Fbar, double* B) {
    const double* apred = F;
    const double* Ppred = apred + (long)R * T * m;
    const double* vs = Ppred + (long)R * T * m * m + (long)R * T * m;
    const double* Fs = vs + (long)R * T;
    double* ybar = B;
    double* hbar = ybar + (long)R * T;
    double* Zbar = hbar + (long)R * T;
    double* Tbar = Zbar + (long)R * T * m;
    double* Qbar = Tbar + m * m;
    double* a0bar = Qbar + m * m;
    double* P0bar = a0bar + m;
    double* part = P0bar + m * m;
    const int PS = 3 * m * m + m;
    double M[MS], K[MS], af[MS], Pf[MS * MS], X[MS * MS], Xb[MS * MS], Pfb[MS * MS], afb[MS], Kb[MS], Mb[MS], ab[MS], Pb[MS * MS], nab[MS],
        nPb[MS * MS];
    (void)y; (void)h; (void)Q;
    for (int r = 0; r < R; ++r) {
        double* Tb = part + (long)r * PS;
        double* Qb = Tb + m * m;
        double* a0b = Qb + m * m;
        double* P0b = a0b + m;
        for (int i = 0; i < m * m; ++i) Tb[i] = Qb[i] = Pb[i] = 0.0;
        for (int i = 0; i < m; ++i) ab[i] = 0.0;
        for (int t = T - 1; t >= 0; --t) {
            const long s = (long)r * T + t;
            const double* z = Z + s * m;
            const double* a = apred + s * m;
            const double* P = Ppred + s * m * m;
            const int seen = !masked || obs[s] != 0.0;
            const double v = vs[s], Fv = Fs[s];
            update(m, seen, a, P, z, v, Fv, M, K, af, Pf);
            if (t < T - 1) {
                for (int i = 0; i < m; ++i)
                    for (int j = 0; j < m; ++j) X[i * m + j] = dotk(Pf + i * m, 1, Tm + j * m, 1, m);
                for (int i = 0; i < m * m; ++i) Qb[i] += Pb[i];
                for (int k = 0; k < m; ++k)
                    for (int j = 0; j < m; ++j) Xb[k * m + j] = dotk(Tm + k, m, Pb + j, m, m);
                for (int i = 0; i < m; ++i)
                    for (int k = 0; k < m; ++k)
                        Tb[i * m + k] = ((Tb[i * m + k] + dotk(Pb + i * m, 1, X + k * m, 1, m)) + dotk(Xb + i, m, Pf + k, m, m)) + ab[i] * af[k];
                for (int i = 0; i < m; ++i)
                    for (int k = 0; k < m; ++k) Pfb[i * m + k] = dotk(Xb + i * m, 1, Tm + k, m, m);
                for (int k = 0; k < m; ++k) afb[k] = dotk(Tm + k, m, ab, 1, m);
            } else {
                for (int i = 0; i < m * m; ++i) Pfb[i] = 0.0;
                for (int i = 0; i < m; ++i) afb[i] = 0.0;
            }
            if (seen) {
                for (int i = 0; i < m; ++i) Kb[i] = afb[i] * v - dotk(Pfb + i * m, 1, M, 1, m);
                const double vb = vbar[s] + dotk(afb, 1, K, 1, m);
                for (int j = 0; j < m; ++j) Mb[j] = -dotk(Pfb + j, m, K, 1, m);
                for (int i = 0; i < m; ++i) Mb[i] = Mb[i] + Kb[i] / Fv;
                const double Fb = Fbar[s] - dotk(Kb, 1, K, 1, m) / Fv;
                hbar[s] = Fb;
                for (int k = 0; k < m; ++k) Mb[k] = fma(Fb, z[k], Mb[k]);
                for (int i = 0; i < m; ++i)
                    for (int k = 0; k < m; ++k) nPb[i * m + k] = fma(Mb[i], z[k], Pfb[i * m + k]);
                for (int k = 0; k < m; ++k) Zbar[s * m + k] = (Fb * M[k] + dotk(P + k, m, Mb, 1, m)) - vb * a[k];
                ybar[s] = vb;
                for (int k = 0; k < m; ++k) nab[k] = fma(-vb, z[k], afb[k]);
            } else {
                for (int i = 0; i < m; ++i) nab[i] = afb[i];
                for (int i = 0; i < m * m; ++i) nPb[i] = Pfb[i];
                ybar[s] = 0.0;
                hbar[s] = 0.0;
                for (int k = 0; k < m; ++k) Zbar[s * m + k] = 0.0;
            }
            for (int i = 0; i < m; ++i) ab[i] = nab[i];
            for (int i = 0; i < m * m; ++i) Pb[i] = nPb[i];
        }
        for (int i = 0; i < m; ++i) a0b[i] = ab[i];
        for (int i = 0; i < m * m; ++i) P0b[i] = Pb[i];
    }
    /* the sums over the series: +0.0 + part_0 + part_1 + ..., ascending r */
    for (int e = 0; e < PS; ++e) {
        double total = 0.0;
        for (int r = 0; r < R; ++r) total = total + part[(long)r * PS + e];
        Tbar[e] = total;       /* Tbar, Qbar, a0bar, P0bar are contiguous, in the partials' order */
    }
}
