/*
 * include/nphip_spec.h compiled for the host and called directly (tests/spec_reference.py builds this with gcc -O2 -ffp-contract=off and loads
 * it through ctypes): the oracle restates the header and the device is compared with the restatement, so this is the only place the header's
 * own text runs on the host.  TEST INFRASTRUCTURE.
 *
 * One record-shaped entry with the fn codes and record shapes of nphip_test_spec (include/nutpie_hip.h): point i reads x[i][0 .. n_in) and
 * writes y[i][0 .. n_out); integers (exponents, Philox words) travel as doubles.  fn 9 (exp_scale_select) exists on the device only: here it is fn 8.
 */
#include "../../include/nphip_spec.h"

int spec_header(int fn, uint64_t n, int n_in, const double* x, int n_out, double* y) {
    static const int shape[17][2] = {{1, 1}, {1, 1}, {1, 1}, {1, 2}, {1, 1}, {2, 1}, {2, 1}, {1, 2}, {1, 1}, {1, 1}, {1, 2}, {3, 1}, {4, 2}, {5, 1}, {4, 2}, {6, 4}, {2, 1}};
    if (fn < 0 || fn > 16 || n_in != shape[fn][0] || n_out != shape[fn][1]) return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const double* a = x + i * (uint64_t)n_in;
        double* o = y + i * (uint64_t)n_out;
        int64_t e;
        switch (fn) {
            case 0: o[0] = nphip_exp(a[0]); break;
            case 1: o[0] = nphip_log(a[0]); break;
            case 2: o[0] = nphip_log1p(a[0]); break;
            case 3: nphip_sincos2pi(a[0], &o[0], &o[1]); break;
            case 4: o[0] = sqrt(a[0]); break;
            case 5: o[0] = a[0] / a[1]; break;
            case 6: o[0] = nphip_logaddexp(a[0], a[1]); break;
            case 7: nphip_exp_parts(a[0], &o[0], &o[1]); break;
            case 8: case 9: {
                const double xv = a[0], xc = xv > 1e9 ? 1e9 : (xv < -1e9 ? -1e9 : xv);
                double p, k;
                nphip_exp_parts(xc, &p, &k);
                o[0] = xv != xv ? p : nphip_exp_scale(xv, p, k);   /* (a NaN comes out of the parts: its k has no integer value on the host) */
                break;
            }
            case 10: nphip_w_leaf(a[0], &o[0], &e); o[1] = (double)e; break;
            case 11: o[0] = nphip_w_rel(a[0], (int64_t)a[1], (int64_t)a[2]); break;
            case 12: nphip_w_add(a[0], (int64_t)a[1], a[2], (int64_t)a[3], &o[0], &e); o[1] = (double)e; break;
            case 13: {
                double sm;
                nphip_w_add(a[1], (int64_t)a[2], a[3], (int64_t)a[4], &sm, &e);
                o[0] = a[0] * sm < nphip_w_rel(a[3], (int64_t)a[4], e) ? 1.0 : 0.0;
                break;
            }
            case 14: {
                nphip_u32x4 r;
                for (int j = 0; j < 4; ++j) r.v[j] = (uint32_t)a[j];
                nphip_normal_pair(r, &o[0], &o[1]);
                break;
            }
            case 15: {
                const uint64_t seed = ((uint64_t)(uint32_t)a[1] << 32) | (uint64_t)(uint32_t)a[0];
                nphip_u32x4 r = nphip_philox(seed, (uint32_t)a[2], (uint32_t)a[3], (uint32_t)a[4], (uint32_t)a[5]);
                for (int j = 0; j < 4; ++j) o[j] = (double)r.v[j];
                break;
            }
            default: o[0] = nphip_u01((uint32_t)a[0], (uint32_t)a[1]); break;
        }
    }
    return 0;
}
