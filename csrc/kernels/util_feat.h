// The feature columns of a packed table (launch.h UtilTable), F = [standardised continuous | one-hot(codes) | 1], as
// the kernels of utility.hip and mlp.hip make them in registers: the one-hot blocks never exist in memory.  Inline
// functions only.
#ifndef FEDTGAN_UTIL_FEAT_H
#define FEDTGAN_UTIL_FEAT_H
#include "common.h"
#include "eval_common.h"
#include "launch.h"

namespace fedtgan {

struct UFeat {
  int kind, col, bin, card;      // kind 0: no feature, 1: continuous column col, 2: one-hot (column col, bin), 3: the 1
};

__device__ __forceinline__ UFeat util_feat(const UtilTable& t, int f) {
  UFeat d{0, 0, 0, 0};
  if (f < 0 || f >= t.D) return d;
  if (f < t.n_cont) {
    d.kind = 1;
    d.col = f;
  } else if (f == t.D - 1) {
    d.kind = 3;
  } else if (t.n_cat > 0) {
    const int wv = f - t.n_cont;
    int lo = 0, hi = t.n_cat - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (t.offs[mid] <= wv) lo = mid; else hi = mid - 1;
    }
    const int k = wv - t.offs[lo], K = t.card[lo];
    if (k >= 0 && k <= K) {
      d.kind = 2;
      d.col = lo;
      d.bin = k;
      d.card = K;
    }
  }
  return d;
}

// (row < t.n is the caller's)
__device__ __forceinline__ double util_fval(const UtilTable& t, const UFeat& d, int row) {
  if (d.kind == 1) return t.cont[(size_t)row * t.n_cont + d.col];
  if (d.kind == 2) return code_clamp(t.cat_t[(size_t)d.col * t.ldk + row], d.card) == d.bin ? 1.0 : 0.0;
  return d.kind == 3 ? 1.0 : 0.0;
}

}  // namespace fedtgan

#endif  // FEDTGAN_UTIL_FEAT_H
