// Device helpers shared by the evaluators that work on label codes and class counts: correlation.hip, utility.hip
// and forest.hip.  Inline functions only, so each translation unit compiles its own copy under its own
// floating-point settings (forest.hip includes this header below its `fp contract(off)`; utility.hip keeps the
// default).
#ifndef FEDTGAN_EVAL_COMMON_H
#define FEDTGAN_EVAL_COMMON_H
#include "common.h"

namespace fedtgan {

// a stored code of a column with K categories: [0, K) is a category, anything else the overflow bin K
__device__ __forceinline__ int code_clamp(int code, int K) { return code < 0 ? K : (code > K ? K : code); }

// a decoded value as such a code (a NaN fails both comparisons)
__device__ __forceinline__ bool is_code(double v, int K) { return v >= 0.0 && v < (double)K; }
__device__ __forceinline__ int code_or_overflow(double v, int K) { return is_code(v, K) ? (int)v : K; }

// the valid rows and the classes present of the class counts (one thread)
__device__ __forceinline__ void class_head(const int* counts, int K, int& n_valid, int& present) {
  int nv = 0, np = 0;
  for (int c = 0; c < K; ++c) {
    nv += counts[c];
    np += counts[c] > 0;
  }
  n_valid = nv;
  present = np;
}

// sklearn's class_weight="balanced" for a class of `count` rows; 0 for an absent class
__device__ __forceinline__ double balanced_weight(int n_valid, int present, int count) {
  return count > 0 ? (double)n_valid / ((double)present * (double)count) : 0.0;
}

// row sums rs, column sums cs and diagonal tp of a [K, K] confusion matrix (one thread, in class order):
// out[0..5] = weighted F1, accuracy, the real fit's two, and the gaps real - fake
__device__ __forceinline__ void confusion_scores(const int* rs, const int* cs, const int* tp, int K,
                                                 const double* real, double* out) {
  long long total = 0, right = 0;
  double f1 = 0.0;
  for (int c = 0; c < K; ++c) {
    total += rs[c];
    right += tp[c];
    const int den = rs[c] + cs[c];            // 2 tp + fp + fn
    if (den > 0) f1 = f1 + (double)rs[c] * ((2.0 * (double)tp[c]) / (double)den);
  }
  f1 = total > 0 ? f1 / (double)total : 0.0;
  const double acc = total > 0 ? (double)right / (double)total : 0.0;
  out[0] = f1;
  out[1] = acc;
  out[2] = real[0];
  out[3] = real[1];
  out[4] = real[0] - f1;
  out[5] = real[1] - acc;
}

}  // namespace fedtgan

#endif  // FEDTGAN_EVAL_COMMON_H
