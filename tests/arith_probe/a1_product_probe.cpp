// Host probe of hc_f64_mulmod_q (csrc/hc_arith.h), the product hc_k_a1p<1> / hc_k_a1g<1> form: TEST INFRASTRUCTURE, compiled by tests/test_a1_fp64_product_cpu.py with the flags of
// the arithmetic probe's host twin. out[i] = the product exactly as the kernels call it: the kernel-plaintext word through hc_f64_from_u, c' as the double it is stored as.
#include <stddef.h>
#include "hc_arith.h"

extern "C" void a1_product_probe(const u64 *k, const double *w, double *out, size_t n, u64 q) {
    const double fq = (double)q, qinv = 1.0 / (double)q;
    for (size_t i = 0; i < n; i++) out[i] = hc_f64_mulmod_q(hc_f64_from_u(k[i]), w[i], fq, qinv);
}
