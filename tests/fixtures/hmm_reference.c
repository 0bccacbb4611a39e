/* The order contract of the HMM stages, restated as plain loops: what tests/test_gpu_hmm_stages.py holds
 * nutpie_amd/csrc/chain_hmm.h to, bit for bit.  Built by tests/hmm_reference.py with -ffp-contract=off.
 *
 * logE: R x T x K row-major; P: K x K row-major; pi: K.
 * F = [alpha: R T K | c: R T | m: R T];  B = [beta: R T K | w: R T K | Pbar: K K | pibar: K]. */
#include "nphip_spec.h"

void hmm_forward(int R, int T, int K, const double* logE, const double* P, const double* pi, double* F) {
    double* alpha = F;
    double* c = F + (long)R * T * K;
    double* m = c + (long)R * T;
    double e[16], a[16];
    for (int r = 0; r < R; ++r) {
        for (int t = 0; t < T; ++t) {
            const double* le = logE + ((long)r * T + t) * K;
            double mx = le[0];
            for (int k = 1; k < K; ++k) mx = (le[k] > mx || le[k] != le[k]) ? le[k] : mx;
            for (int k = 0; k < K; ++k) e[k] = nphip_exp(le[k] - mx);
            if (t == 0) {
                for (int j = 0; j < K; ++j) a[j] = pi[j] * e[j];
            } else {
                const double* prev = alpha + ((long)r * T + t - 1) * K;
                for (int j = 0; j < K; ++j) {
                    double acc = 0.0;
                    for (int i = 0; i < K; ++i) acc = fma(prev[i], P[i * K + j], acc);
                    a[j] = acc * e[j];
                }
            }
            double sum = 0.0;
            for (int j = 0; j < K; ++j) sum = sum + a[j];
            for (int j = 0; j < K; ++j) alpha[((long)r * T + t) * K + j] = a[j] / sum;
            c[(long)r * T + t] = sum;
            m[(long)r * T + t] = mx;
        }
    }
}

void hmm_backward(int R, int T, int K, const double* logE, const double* P, const double* F, double* B) {
    const double* alpha = F;
    const double* c = F + (long)R * T * K;
    const double* m = c + (long)R * T;
    double* beta = B;
    double* w = B + (long)R * T * K;
    double* Pbar = w + (long)R * T * K;
    double* pibar = Pbar + K * K;
    for (int r = 0; r < R; ++r) {
        for (int i = 0; i < K; ++i) beta[((long)r * T + T - 1) * K + i] = 1.0;
        for (int t = T - 1; t >= 0; --t) {
            const long row = ((long)r * T + t) * K;
            for (int j = 0; j < K; ++j) w[row + j] = (nphip_exp(logE[row + j] - m[(long)r * T + t]) * beta[row + j]) / c[(long)r * T + t];
            if (t > 0) {
                for (int i = 0; i < K; ++i) {
                    double acc = 0.0;
                    for (int j = 0; j < K; ++j) acc = fma(P[i * K + j], w[row + j], acc);
                    beta[row - K + i] = acc;
                }
            }
        }
    }
    for (int i = 0; i < K; ++i) {
        for (int j = 0; j < K; ++j) {
            double total = 0.0;
            for (int r = 0; r < R; ++r) {
                double s = 0.0;
                for (int t = 1; t < T; ++t) s = fma(alpha[((long)r * T + t - 1) * K + i], w[((long)r * T + t) * K + j], s);
                total = total + s;
            }
            Pbar[i * K + j] = total;
        }
    }
    for (int k = 0; k < K; ++k) {
        double total = 0.0;
        for (int r = 0; r < R; ++r) total = total + w[(long)r * T * K + k];
        pibar[k] = total;
    }
}
