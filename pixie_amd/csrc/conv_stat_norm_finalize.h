// pixie_amd/csrc/conv_stat_norm_finalize.h -- FRAGMENT of stats_norm_finalize_kernel and of its grouped twin (conv_stat_kernels.h),
// included inside each as its statements (textual inclusion for the reason conv16_body.h gives: the same statements behind a
// __forceinline__ function compile to different code for the single form).  No include guard: included once per kernel.
//   names read:   P0, sums0, c0, P1, sums1, channels, spatial, mode, groups, eps, weight, bias, a, b
//   writes:       sums0 / sums1 (the parts whose partials it adds up), a, b; LDS: r[8]
    __shared__ double r[8];
    const int cpg = mode == 0 ? 1 : channels / groups;
    const int first = blockIdx.x * cpg;
    double s1 = 0.0, s2 = 0.0;
    for (int k = first; k < first + cpg; ++k) {
        const bool in0 = k < c0;
        const StatParts& P = in0 ? P0 : P1;
        double* sums = in0 ? sums0 : sums1;
        const int kc = in0 ? k : k - c0;
        double t1, t2;
        if (P.n > 0) {
            block_channel_sums(P, kc, r, t1, t2);
            if (threadIdx.x == 0) { sums[2 * kc] = t1; sums[2 * kc + 1] = t2; }
        } else {
            t1 = sums[2 * kc]; t2 = sums[2 * kc + 1];
        }
        s1 += t1; s2 += t2;
    }
    const double cnt = mode == 0 ? spatial : spatial * cpg;
    const double mean = s1 / cnt;
    double var = s2 / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + eps);
    for (int k = first + threadIdx.x; k < first + cpg; k += 256) {
        if (mode == 0) {
            a[k] = (float)rstd;
            b[k] = (float)(-mean * rstd);
        } else {
            const double w = weight ? (double)weight[k] : 1.0;
            const double bb = bias ? (double)bias[k] : 0.0;
            a[k] = (float)(rstd * w);
            b[k] = (float)(bb - mean * rstd * w);
        }
    }
