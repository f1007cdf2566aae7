// Flip test: the two launches around the second forward of HRNet's / Simple Baselines' TEST.FLIP_TEST --
// mirror the input batch, then flip the second output back (columns reversed, left/right channels swapped, optionally moved one
// column to the right: TEST.SHIFT_HEATMAP), average it with the first and keep the arg-max keys of what is stored.
// Both are streaming kernels, HBM-bound, no LDS: a wave that reads 64 consecutive floats in reverse order touches the same
// cache lines as in forward order, so plain per-lane loads of the mirrored address coalesce, with or without the shift.
// 64-bit indexing throughout.
#include "mval_common.h"

// out[r][x] = in[r][W - 1 - x]: a bit copy (32-bit words, no float operation touches the values)
__global__ __launch_bounds__(256) void mirror_images_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t total, int W) {
  // (one 64-bit division per thread, not per element: the row and column advance by the stride's quotient and remainder)
  const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t step_rows = step / W;
  const int step_cols = (int)(step - step_rows * W);
  int64_t row0 = first / W * W;  // flat index of the row's first element
  int x = (int)(first - row0);
  for (int64_t i = first; i < total; i += step) {
    out[i] = in[row0 + (W - 1 - x)];
    row0 += step_rows * W;
    x += step_cols;
    if (x >= W) {
      x -= W;
      row0 += W;
    }
  }
}

extern "C" int mval_mirror_images(const float* in, float* out, int64_t n_rows, int W, void* stream) {
  MVAL_REQUIRE(n_rows >= 0 && W >= 1, "mval_mirror_images: bad dims");
  if (n_rows == 0) return 0;
  MVAL_REQUIRE(in && out, "mval_mirror_images: in and out must not be NULL");
  MVAL_REQUIRE(n_rows <= (int64_t)0x7fffffffffffffffll / 4 / W, "mval_mirror_images: too many elements");
  const int64_t total = n_rows * W;
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, bytes = (uintptr_t)total * 4;
  MVAL_REQUIRE(a + bytes <= b || b + bytes <= a, "mval_mirror_images: out must not alias in");
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(mirror_images_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, mval_stream(stream),
                     reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), total, W);
  MVAL_CHECK_LAUNCH("mval_mirror_images");
  return 0;
}

// One 256-thread workgroup per (image, joint) map, flat-index loop (wh is 48, 64 or 72 in the project's configs: no
// row-per-wave assumption).  Every thread keeps the best key of what it stored -- its indices ascend, and the key's low word
// is ~index, so the first of equal values wins --, the wave reduces by shuffles and lane 0 stores the wave's key in slot
// `wave` of the map.  Lanes 1..31 of the four waves store the zeros of slots 4..127, so the keys need no clear beforehand
// and no atomics.  A wave whose part of a small map is empty stores 0, an unused slot's value (every stored value has a key > 0).
template <int SHIFT>
__global__ __launch_bounds__(256) void flip_merge_kernel(const float* __restrict__ hm, const float* __restrict__ hm_mirrored,
                                                         const int32_t* __restrict__ pairs, float* __restrict__ merged,
                                                         unsigned long long* __restrict__ keys, int J, int hh, int wh) {
  const int64_t map = blockIdx.x;
  const int64_t n = map / J;
  const int j = (int)(map - n * J);
  int p = pairs[j];
  if ((unsigned)p >= (unsigned)J) p = j;  // (a device array cannot be refused on the host: no read outside the tensor)
  const int npix = hh * wh;
  const float* __restrict__ a = hm + map * npix;
  const float* __restrict__ b = hm_mirrored + (n * J + p) * npix;
  float* __restrict__ o = merged + map * npix;
  unsigned long long best = 0ull;
  const int step_rows = 256 / wh, step_cols = 256 - step_rows * wh;  // (one division per thread: row and column advance with the stride)
  int row0 = (int)threadIdx.x / wh * wh;  // flat index of the row's first element
  int x = (int)threadIdx.x - row0;
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int xm = SHIFT ? min(wh - x, wh - 1) : wh - 1 - x;
    const float v = __fmul_rn(__fadd_rn(a[i], b[row0 + xm]), 0.5f);  // one add, one halving: what a float32 host oracle computes
    o[i] = v;
    const unsigned long long k = mval_argmax_key(v, (unsigned)i);
    best = k > best ? k : best;
    row0 += step_rows * wh;
    x += step_cols;
    if (x >= wh) {
      x -= wh;
      row0 += wh;
    }
  }
  if (!keys) return;
  best = mval_key_group_max(best, 32);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  static_assert(MVAL_ARGMAX_SLOTS == 4 + 4 * 31, "lanes 1..31 of four waves cover the unused slots");
  if (lane < 32) {
    const int slot = lane == 0 ? wave : 4 + wave * 31 + (lane - 1);
    keys[(n * MVAL_ARGMAX_SLOTS + slot) * J + j] = lane == 0 ? best : 0ull;  // [image][slot][joint]
  }
}

extern "C" int mval_flip_merge_heatmaps(const float* hm, const float* hm_mirrored, const int32_t* pairs, int shift, float* merged,
                                        uint64_t* argmax_keys, int64_t N, int J, int hh, int wh, void* stream) {
  // (a flat index is the low word of a key and goes through an int: the limit of mval_pred_coordinates_from_keys)
  MVAL_REQUIRE(N >= 0 && J >= 1 && hh >= 1 && wh >= 1 && (int64_t)hh * wh < (1 << 24), "mval_flip_merge_heatmaps: bad dims");
  if (N == 0) return 0;
  MVAL_REQUIRE(hm && hm_mirrored && pairs && merged, "mval_flip_merge_heatmaps: hm, hm_mirrored, pairs and merged must not be NULL");
  MVAL_REQUIRE(N <= 0x7fffffff / (int64_t)J, "mval_flip_merge_heatmaps: too many maps");
  const uintptr_t bytes = (uintptr_t)(N * J) * (uintptr_t)(hh * wh) * 4, m = (uintptr_t)merged;
  MVAL_REQUIRE((m + bytes <= (uintptr_t)hm || (uintptr_t)hm + bytes <= m) &&
                   (m + bytes <= (uintptr_t)hm_mirrored || (uintptr_t)hm_mirrored + bytes <= m),
               "mval_flip_merge_heatmaps: merged must alias neither hm nor hm_mirrored");
  MVAL_REQUIRE(((uintptr_t)argmax_keys & 7) == 0, "mval_flip_merge_heatmaps: argmax_keys must be 8-byte aligned");
  const dim3 grid((unsigned)(N * J));
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(argmax_keys);
  if (shift)
    hipLaunchKernelGGL(flip_merge_kernel<1>, grid, dim3(256), 0, mval_stream(stream), hm, hm_mirrored, pairs, merged, keys, J, hh, wh);
  else
    hipLaunchKernelGGL(flip_merge_kernel<0>, grid, dim3(256), 0, mval_stream(stream), hm, hm_mirrored, pairs, merged, keys, J, hh, wh);
  MVAL_CHECK_LAUNCH("mval_flip_merge_heatmaps");
  return 0;
}
