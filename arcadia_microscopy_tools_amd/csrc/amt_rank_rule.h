// The rank rule of np.percentile, method 'linear', for selections whose count is only known on the device (no HIP here:
// a host compiler can test it; under hipcc the functions are __host__ __device__).
//   virtual index v = (n - 1) * q / 100; lo = floor(v), hi = lo + 1, t = v - lo; the ends (v >= n - 1, v < 0) take one
//   rank twice with t = 0                                  (amt_stats.hip's make_rank_reqs, which keeps its own copy)
//   numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) for t >= 0.5                   (amt_stats.hip's np_lerp)
// For uint16 values and q = 25 / 50 / 75 the weight is a whole number of quarters and every result is a multiple of 1/4
// far below 2^53: the integer forms below give numpy's float64 bits whatever the order of evaluation.
#pragma once

#if defined(__HIPCC__)
#define AMT_RULE_FN __host__ __device__ static inline
#else
#define AMT_RULE_FN static inline
#endif

struct amt_rank {
    unsigned long long lo, hi;  // 0-based ranks in ascending order; hi <= n - 1
    double t;                   // weight of the value of rank hi
};

// ranks and weight of the quantile `quant` (= q / 100, in 0..1) among n >= 1 values
AMT_RULE_FN amt_rank amt_rank_of(unsigned long long n, double quant) {
    amt_rank r;
    const double last = (double)(n - 1), v = last * quant;
    if (v >= last) {
        r.lo = r.hi = n - 1;
        r.t = 0.0;
    } else if (v < 0) {
        r.lo = r.hi = 0;
        r.t = 0.0;
    } else {
        const double f = __builtin_floor(v);
        r.lo = (unsigned long long)f;
        r.hi = r.lo + 1;  // < n: v < n - 1
        r.t = v - f;
    }
    return r;
}

AMT_RULE_FN double amt_np_lerp(double a, double b, double t) {
    const double d = b - a;
    double r = a + d * t;
    if (t >= 0.5) r = b - d * (1.0 - t);
    return r;
}

// ---- uint16 values, q = 25 / 50 / 75 ----------------------------------------------------------------------------
// the weight in quarters: t is 0, 1/4, 1/2 or 3/4 exactly ((n - 1) / 4, / 2, * 3 / 4 are exact in float64)
AMT_RULE_FN int amt_rank_quarters(double t) { return (int)(t * 4.0); }

// the quantile from the values a <= b of ranks lo / hi and the weight t4 / 4
AMT_RULE_FN double amt_quartile_u16(unsigned a, unsigned b, int t4) {
    return (double)(4ll * (long long)a + (long long)(b - a) * t4) * 0.25;
}

// 2 * median from the values a <= b of the median's ranks: the median is a for an odd count, (a + b) / 2 for an even one
AMT_RULE_FN unsigned amt_median2_u16(unsigned a, unsigned b, bool n_odd) { return n_odd ? 2u * a : a + b; }

// MAD from the keys ka <= kb of the median's ranks among the keys |2 v - 2 median| (twice the distances)
AMT_RULE_FN double amt_mad_u16(unsigned ka, unsigned kb, bool n_odd) {
    return n_odd ? (double)ka * 0.5 : (double)((unsigned long long)ka + kb) * 0.25;
}
