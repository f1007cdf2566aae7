// The training split's RandAugment on the device (the reference's dataset/augmentation.py, called from
// dataset/dataset.py:212-213 between the LANCZOS resize and the normalisation): Pillow's ImageOps / ImageEnhance /
// Image.rotate on a batch of V uint8 views [V][H][W][3], bit for bit (Pillow 12.2.0; tests/golden/augment.npz).
//
// Every view has its own list of K ops ([V][K] descriptors in device memory); at step k the views run different ops.  A
// workgroup belongs to one view, reads that view's kind and leaves when the pass is not its own, so a step costs one launch
// per KIND OF PASS some view needs (the host knows the kinds present per step), whatever V is:
//   statistics   per-(view, channel) histograms in LDS, merged with atomics, + the integer sum of L   (AutoContrast, Equalize, Contrast)
//   tables       256 entries per (view, channel): Invert, Solarize, Posterize, AutoContrast, Equalize, Brightness, Contrast
//   apply        the table pass
//   colour       blend(L, image, f) per pixel
//   spatial      Sharpness (3x3 SMOOTH + blend) and Rotate (bicubic gather), image -> second buffer
//   copy back    second buffer -> image for the views of the spatial pass
// The target side of Rotate (mval_rotate_maps, at the end of the file) turns the float32 heat-maps of the rotated views the same way.
// Rounding: Pillow's C evaluates the blends and the 3x3 filter in float32 and the bicubic transform in float64, one rounding
// per operation; hipcc contracts a * b + c to an FMA by default, so this file switches contraction off (see below).
// Pixels are 3 bytes: a thread owns 4 consecutive pixels (12 bytes = 3 dwords) or 4 consecutive bytes, so that a wave's
// loads are consecutive dwords wherever a view starts on a dword (H * W * 3 a multiple of 4: every network input in use);
// other views take the same code with byte accesses.
#include "mval_common.h"

// The __fmul_rn / __dadd_rn family is plain `x * y` / `x + y` in this toolchain's headers and fuses like any other expression once
// inlined, so contraction is switched off for the whole file and the rounded operations are spelt out through the helpers below.
#pragma clang fp contract(off)
__device__ __forceinline__ float aug_fmul(float a, float b) { return a * b; }
__device__ __forceinline__ float aug_fadd(float a, float b) { return a + b; }
__device__ __forceinline__ double aug_dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double aug_dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double aug_ddiv(double a, double b) { return a / b; }

#define AUG_BIT(k) (1u << (k))
#define AUG_STATS_KINDS (AUG_BIT(MVAL_AUG_AUTOCONTRAST) | AUG_BIT(MVAL_AUG_EQUALIZE) | AUG_BIT(MVAL_AUG_CONTRAST))
#define AUG_TABLE_KINDS (AUG_STATS_KINDS | AUG_BIT(MVAL_AUG_INVERT) | AUG_BIT(MVAL_AUG_POSTERIZE) | AUG_BIT(MVAL_AUG_SOLARIZE) | AUG_BIT(MVAL_AUG_BRIGHTNESS))
#define AUG_SPATIAL_KINDS (AUG_BIT(MVAL_AUG_SHARPNESS) | AUG_BIT(MVAL_AUG_ROTATE))
#define AUG_STATS_ITERS 4  // groups of 4 pixels per thread of the statistics pass: 4096 pixels per workgroup
#define AUG_APPLY_ITERS 4  // dwords per thread of the table / copy passes: 4096 bytes per workgroup

__device__ __forceinline__ bool aug_is(unsigned kinds, int kind) { return kind >= 0 && kind < 32 && ((kinds >> kind) & 1u); }

// ImagingBlend / the filters' clip: 0 at or below 0, 255 at or above 255, truncation between
__device__ __forceinline__ int aug_clip(float t) { return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t; }
__device__ __forceinline__ int aug_clip(double t) { return t <= 0.0 ? 0 : t >= 255.0 ? 255 : (int)t; }
// Image.blend(a, b, f): a + f * (b - a) in float32, the product and the sum rounded separately
__device__ __forceinline__ int aug_blend(int a, int b, float f) { return aug_clip(aug_fadd((float)a, aug_fmul(f, (float)(b - a)))); }
// convert("L"): ITU-R 601-2 luma in 16-bit fixed point, on channel POSITIONS
__device__ __forceinline__ int aug_luma(int c0, int c1, int c2) { return (19595 * c0 + 38470 * c1 + 7471 * c2 + 32768) >> 16; }

// pixels 4q .. 4q + 3 of a view: three dword loads where the view starts on a dword and all four pixels exist
__device__ __forceinline__ int aug_load4(const unsigned char* view, int q, int npix, bool dw, unsigned char px[12]) {
  const int n = min(4, npix - 4 * q);
  const unsigned char* p = view + (int64_t)q * 12;
  if (dw && n == 4) {
    const unsigned* w = reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const unsigned u = w[j];
      px[j * 4] = u & 255u, px[j * 4 + 1] = (u >> 8) & 255u, px[j * 4 + 2] = (u >> 16) & 255u, px[j * 4 + 3] = u >> 24;
    }
  } else {
    for (int j = 0; j < n * 3; j++) px[j] = p[j];
  }
  return n;
}
__device__ __forceinline__ void aug_store4(unsigned char* view, int q, int n, bool dw, const unsigned char px[12]) {
  unsigned char* p = view + (int64_t)q * 12;
  if (dw && n == 4) {
    unsigned* w = reinterpret_cast<unsigned*>(p);
#pragma unroll
    for (int j = 0; j < 3; j++) w[j] = (unsigned)px[j * 4] | ((unsigned)px[j * 4 + 1] << 8) | ((unsigned)px[j * 4 + 2] << 16) | ((unsigned)px[j * 4 + 3] << 24);
  } else {
    for (int j = 0; j < n * 3; j++) p[j] = px[j];
  }
}

// ---- statistics: Image.histogram() per channel and sum(convert("L")) ---------------------------------------------------------
// grid (ceil(npix / 4096), V) x 256 threads.  hist [V][3][256], lsum [V], both zeroed before the launch.
__global__ __launch_bounds__(256) void aug_stats_kernel(const unsigned char* __restrict__ img, const mval_aug_op* __restrict__ ops, int n_steps,
                                                        int step, int npix, unsigned* __restrict__ hist, unsigned long long* __restrict__ lsum) {
  const int v = blockIdx.y;
  if (!aug_is(AUG_STATS_KINDS, ops[(int64_t)v * n_steps + step].kind)) return;  // uniform per workgroup
  __shared__ unsigned h_s[3 * 256];
  __shared__ unsigned l_s;
  for (int i = threadIdx.x; i < 3 * 256; i += 256) h_s[i] = 0;
  if (threadIdx.x == 0) l_s = 0;
  __syncthreads();
  const unsigned char* view = img + (int64_t)v * npix * 3;
  const bool dw = (reinterpret_cast<uintptr_t>(view) & 3) == 0;
  unsigned l = 0;
  for (int it = 0; it < AUG_STATS_ITERS; it++) {
    const int q = (blockIdx.x * AUG_STATS_ITERS + it) * 256 + threadIdx.x;
    if (4 * q >= npix) break;
    unsigned char px[12];
    const int n = aug_load4(view, q, npix, dw, px);
    for (int j = 0; j < n; j++) {
      atomicAdd(&h_s[px[j * 3]], 1u);
      atomicAdd(&h_s[256 + px[j * 3 + 1]], 1u);
      atomicAdd(&h_s[512 + px[j * 3 + 2]], 1u);
      l += aug_luma(px[j * 3], px[j * 3 + 1], px[j * 3 + 2]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&l_s, l);  // (at most 4096 * 255 per workgroup)
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += 256)
    if (h_s[i]) atomicAdd(&hist[(int64_t)v * 768 + i], h_s[i]);
  if (threadIdx.x == 0) atomicAdd(&lsum[v], (unsigned long long)l_s);
}

// ---- tables: lut [V][3][256], thread i of workgroup v writes entry i of the three channels ------------------------------------
__global__ __launch_bounds__(256) void aug_table_kernel(const mval_aug_op* __restrict__ ops, int n_steps, int step, int npix,
                                                        const unsigned* __restrict__ hist, const unsigned long long* __restrict__ lsum,
                                                        unsigned char* __restrict__ lut) {
  const int v = blockIdx.x, i = threadIdx.x;
  const mval_aug_op op = ops[(int64_t)v * n_steps + step];
  if (!aug_is(AUG_TABLE_KINDS, op.kind)) return;
  __shared__ unsigned h_s[3 * 256];
  if (aug_is(AUG_STATS_KINDS, op.kind)) {
    for (int j = i; j < 3 * 256; j += 256) h_s[j] = hist[(int64_t)v * 768 + j];
    __syncthreads();  // (the kind is uniform per workgroup)
  }
  const double val = op.p[0];
  for (int c = 0; c < 3; c++) {
    const unsigned* h = h_s + c * 256;
    int l = i;
    switch (op.kind) {
      case MVAL_AUG_INVERT: l = 255 - i; break;
      case MVAL_AUG_SOLARIZE: l = (double)i < val ? i : 255 - i; break;
      case MVAL_AUG_POSTERIZE: {
        int bits = (int)val;  // the reference: max(1, int(v)); ImageOps.posterize: i & ~(2 ** (8 - bits) - 1)
        bits = bits < 1 ? 1 : bits > 8 ? 8 : bits;
        l = i & ~((1 << (8 - bits)) - 1);
        break;
      }
      case MVAL_AUG_BRIGHTNESS: l = aug_blend(0, i, (float)val); break;
      case MVAL_AUG_CONTRAST: {  // the degenerate image is the constant int(mean(L) + 0.5), the mean a float64 quotient of integers
        const int m = (int)aug_dadd(aug_ddiv((double)lsum[v], (double)npix), 0.5);
        l = aug_blend(m, i, (float)val);
        break;
      }
      case MVAL_AUG_AUTOCONTRAST: {  // ImageOps.autocontrast(cutoff=0): first and last non-empty bin
        int lo = 256, hi = -1;
        for (int j = 0; j < 256; j++)
          if (h[j]) {
            if (lo == 256) lo = j;
            hi = j;
          }
        if (hi > lo) {
          const double scale = aug_ddiv(255.0, (double)(hi - lo)), offset = aug_dmul(-(double)lo, scale);
          const double t = aug_dadd(aug_dmul((double)i, scale), offset);
          l = t < 0.0 ? 0 : t > 255.0 ? 255 : (int)t;  // int() truncates toward zero, then the clamp
          l = l < 0 ? 0 : l > 255 ? 255 : l;
        }
        break;
      }
      case MVAL_AUG_EQUALIZE: {  // ImageOps.equalize: step from the non-empty bins but the last, running sum over ALL bins
        unsigned total = 0, last = 0, before = 0;
        int nonempty = 0;
        for (int j = 0; j < 256; j++) {
          const unsigned hj = h[j];
          if (hj) nonempty++, total += hj, last = hj;
          if (j < i) before += hj;
        }
        const unsigned st = (total - last) / 255u;
        if (nonempty > 1 && st != 0) {
          const unsigned e = (st / 2 + before) / st;
          l = e > 255u ? 255 : (int)e;  // Image.point clips the table's entries to 8 bits
        }
        break;
      }
      default: break;
    }
    lut[((int64_t)v * 3 + c) * 256 + i] = (unsigned char)l;
  }
}

// ---- apply: byte b of a view is channel b % 3.  grid (ceil(H * W * 3 / 4096), V) x 256 ---------------------------------------
__global__ __launch_bounds__(256) void aug_apply_kernel(unsigned char* __restrict__ img, const mval_aug_op* __restrict__ ops, int n_steps, int step,
                                                        int nbytes, const unsigned char* __restrict__ lut) {
  const int v = blockIdx.y;
  if (!aug_is(AUG_TABLE_KINDS, ops[(int64_t)v * n_steps + step].kind)) return;
  __shared__ unsigned char lut_s[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) lut_s[i] = lut[(int64_t)v * 768 + i];
  __syncthreads();
  unsigned char* view = img + (int64_t)v * nbytes;
  const bool dw = (reinterpret_cast<uintptr_t>(view) & 3) == 0;
  for (int it = 0; it < AUG_APPLY_ITERS; it++) {
    const int b0 = ((blockIdx.x * AUG_APPLY_ITERS + it) * 256 + threadIdx.x) * 4;
    if (b0 >= nbytes) break;
    int c = b0 % 3;
    if (dw && b0 + 4 <= nbytes) {
      const unsigned u = *reinterpret_cast<const unsigned*>(view + b0);
      unsigned o = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        o |= (unsigned)lut_s[c * 256 + ((u >> (8 * j)) & 255u)] << (8 * j);
        c = c == 2 ? 0 : c + 1;
      }
      *reinterpret_cast<unsigned*>(view + b0) = o;
    } else {
      for (int j = 0; j < 4 && b0 + j < nbytes; j++) {
        view[b0 + j] = lut_s[c * 256 + view[b0 + j]];
        c = c == 2 ? 0 : c + 1;
      }
    }
  }
}

// ---- ImageEnhance.Color: blend(convert("L") on the three channels, image, f).  grid (ceil(npix / 1024), V) x 256 -----------------
__global__ __launch_bounds__(256) void aug_color_kernel(unsigned char* __restrict__ img, const mval_aug_op* __restrict__ ops, int n_steps, int step,
                                                        int npix) {
  const int v = blockIdx.y;
  const mval_aug_op* op = ops + (int64_t)v * n_steps + step;
  if (op->kind != MVAL_AUG_COLOR) return;
  const float f = (float)op->p[0];
  unsigned char* view = img + (int64_t)v * npix * 3;
  const bool dw = (reinterpret_cast<uintptr_t>(view) & 3) == 0;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (4 * q >= npix) return;
  unsigned char px[12];
  const int n = aug_load4(view, q, npix, dw, px);
  for (int j = 0; j < n; j++) {
    const int g = aug_luma(px[j * 3], px[j * 3 + 1], px[j * 3 + 2]);
#pragma unroll
    for (int c = 0; c < 3; c++) px[j * 3 + c] = (unsigned char)aug_blend(g, px[j * 3 + c], f);
  }
  aug_store4(view, q, n, dw, px);
}

// ---- spatial: one thread per output pixel, image -> second buffer.  grid (ceil(npix / 256), V) x 256 ------------------------------
// Geometry.c BICUBIC: the four taps v1..v4 at fraction d, every operation rounded on its own
__device__ __forceinline__ double aug_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p2 = aug_dadd(-v1, v3);
  const double p3 = aug_dadd(aug_dadd(aug_dmul(2.0, aug_dadd(v1, -v2)), v3), -v4);
  const double p4 = aug_dadd(aug_dadd(aug_dadd(-v1, v2), -v3), v4);
  return aug_dadd(v2, aug_dmul(d, aug_dadd(p2, aug_dmul(d, aug_dadd(p3, aug_dmul(d, p4))))));
}
// one row of ImagingFilter3x3's sum: (a * k0 + b * k1) + c * k2 in float32
__device__ __forceinline__ float aug_row3(const unsigned char* p, float ka, float kb) {
  return aug_fadd(aug_fadd(aug_fmul((float)p[-3], ka), aug_fmul((float)p[0], kb)), aug_fmul((float)p[3], ka));
}

__global__ __launch_bounds__(256) void aug_spatial_kernel(const unsigned char* __restrict__ img, const mval_aug_op* __restrict__ ops, int n_steps,
                                                          int step, int H, int W, unsigned char* __restrict__ out) {
  const int v = blockIdx.y;
  const mval_aug_op* op = ops + (int64_t)v * n_steps + step;
  const int kind = op->kind;
  if (!aug_is(AUG_SPATIAL_KINDS, kind)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const unsigned char* src = img + (int64_t)v * H * W * 3;
  unsigned char* o = out + ((int64_t)v * H * W + i) * 3;
  if (kind == MVAL_AUG_SHARPNESS) {
    // ImageEnhance.Sharpness: blend(filter(SMOOTH), image, f); SMOOTH = (1 1 1 / 1 5 1 / 1 1 1) / 13 as float32 weights, summed from 0.5 over
    // the rows y + 1, y, y - 1; ImagingFilter3x3 copies the one-pixel border (blending a pixel with itself leaves it, whatever f)
    const unsigned char* p = src + (int64_t)i * 3;
    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {
      o[0] = p[0], o[1] = p[1], o[2] = p[2];
      return;
    }
    const float f = (float)op->p[0], k1 = 1.f / 13.f, k5 = 5.f / 13.f;
    const int row = W * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float ss = 0.5f;
      ss = aug_fadd(ss, aug_row3(p + row + c, k1, k1));
      ss = aug_fadd(ss, aug_row3(p + c, k1, k5));
      ss = aug_fadd(ss, aug_row3(p - row + c, k1, k1));
      o[c] = (unsigned char)aug_blend(aug_clip(ss), p[c], f);
    }
    return;
  }
  // Image.rotate(angle, BICUBIC): ImagingGenericTransform with affine_transform and bicubic_filter32RGB, all float64
  const double xc = x + 0.5, yc = y + 0.5;
  double xin = aug_dadd(aug_dadd(aug_dmul(op->p[0], xc), aug_dmul(op->p[1], yc)), op->p[2]);
  double yin = aug_dadd(aug_dadd(aug_dmul(op->p[3], xc), aug_dmul(op->p[4], yc)), op->p[5]);
  if (!(xin >= 0.0 && yin >= 0.0 && xin < (double)W && yin < (double)H)) {  // outside (or not a number): the fill colour
    o[0] = o[1] = o[2] = 0;
    return;
  }
  xin = aug_dadd(xin, -0.5);
  yin = aug_dadd(yin, -0.5);
  const int fx = (int)floor(xin), fy = (int)floor(yin);
  const double dx = aug_dadd(xin, -(double)fx), dy = aug_dadd(yin, -(double)fy);
  int xs[4], ys[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    xs[t] = min(max(fx - 1 + t, 0), W - 1) * 3;
    ys[t] = min(max(fy - 1 + t, 0), H - 1);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double r[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const unsigned char* p = src + (int64_t)ys[t] * W * 3 + c;
      r[t] = aug_cubic((double)p[xs[0]], (double)p[xs[1]], (double)p[xs[2]], (double)p[xs[3]], dx);
    }
    o[c] = (unsigned char)aug_clip(aug_cubic(r[0], r[1], r[2], r[3], dy));
  }
}

// second buffer -> image for the views of the spatial pass.  grid (ceil(H * W * 3 / 4096), V) x 256
__global__ __launch_bounds__(256) void aug_copy_back_kernel(unsigned char* __restrict__ img, const mval_aug_op* __restrict__ ops, int n_steps, int step,
                                                            int nbytes, const unsigned char* __restrict__ buf) {
  const int v = blockIdx.y;
  if (!aug_is(AUG_SPATIAL_KINDS, ops[(int64_t)v * n_steps + step].kind)) return;
  unsigned char* dst = img + (int64_t)v * nbytes;
  const unsigned char* src = buf + (int64_t)v * nbytes;
  const bool dw = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 3) == 0;
  for (int it = 0; it < AUG_APPLY_ITERS; it++) {
    const int b0 = ((blockIdx.x * AUG_APPLY_ITERS + it) * 256 + threadIdx.x) * 4;
    if (b0 >= nbytes) break;
    if (dw && b0 + 4 <= nbytes) *reinterpret_cast<unsigned*>(dst + b0) = *reinterpret_cast<const unsigned*>(src + b0);
    else
      for (int j = 0; j < 4 && b0 + j < nbytes; j++) dst[b0 + j] = src[b0 + j];
  }
}

// workspace: [V] u64 L sums | [V][3][256] u32 histograms | [V][3][256] u8 tables | (256-byte aligned) [V][H][W][3] second buffer
static size_t aug_stats_bytes(int n_views) { return (size_t)n_views * (8 + 768 * 4); }
static size_t aug_buf_offset(int n_views) { return (aug_stats_bytes(n_views) + (size_t)n_views * 768 + 255) & ~(size_t)255; }

extern "C" size_t mval_augment_views_workspace_bytes(int n_views, int h, int w) {
  if (n_views <= 0 || h <= 0 || w <= 0) return 0;
  return aug_buf_offset(n_views) + (size_t)n_views * h * w * 3;
}

extern "C" int mval_augment_views(uint8_t* img, const mval_aug_op* ops, const uint32_t* step_kinds, int n_views, int n_steps, int h, int w,
                                  void* ws, void* stream) {
  MVAL_REQUIRE(img && ops && step_kinds && ws && n_views > 0 && n_steps > 0 && h > 0 && w > 0, "mval_augment_views: bad arguments");
  MVAL_REQUIRE(n_views <= 65535, "mval_augment_views: %d views, at most 65535 per call", n_views);
  MVAL_REQUIRE((int64_t)h * w * 3 <= (int64_t)1 << 30, "mval_augment_views: a %d x %d view is too large", h, w);
  const uint32_t known = AUG_BIT(MVAL_AUG_NONE) | AUG_TABLE_KINDS | AUG_BIT(MVAL_AUG_COLOR) | AUG_SPATIAL_KINDS;
  for (int k = 0; k < n_steps; k++)
    MVAL_REQUIRE(step_kinds[k] != 0 && (step_kinds[k] & ~known) == 0, "mval_augment_views: step %d names unknown kinds (mask 0x%x)", k, step_kinds[k]);
  hipStream_t s = mval_stream(stream);
  const int npix = h * w, nbytes = npix * 3;
  char* base = reinterpret_cast<char*>(ws);
  unsigned long long* lsum = reinterpret_cast<unsigned long long*>(base);
  unsigned* hist = reinterpret_cast<unsigned*>(base + (size_t)n_views * 8);
  unsigned char* lut = reinterpret_cast<unsigned char*>(base + aug_stats_bytes(n_views));
  unsigned char* buf = reinterpret_cast<unsigned char*>(base + aug_buf_offset(n_views));
  const dim3 blk(256);
  const dim3 g_bytes((nbytes + 256 * 4 * AUG_APPLY_ITERS - 1) / (256 * 4 * AUG_APPLY_ITERS), n_views);
  for (int k = 0; k < n_steps; k++) {
    const uint32_t kinds = step_kinds[k];
    if (kinds & AUG_STATS_KINDS) {
      if (hipMemsetAsync(base, 0, aug_stats_bytes(n_views), s) != hipSuccess) {
        mval_set_error("mval_augment_views: clearing the statistics failed");
        return -2;
      }
      hipLaunchKernelGGL(aug_stats_kernel, dim3((npix + 1024 * AUG_STATS_ITERS - 1) / (1024 * AUG_STATS_ITERS), n_views), blk, 0, s, img, ops, n_steps, k,
                         npix, hist, lsum);
      MVAL_CHECK_LAUNCH("mval_augment_views/stats");
    }
    if (kinds & AUG_TABLE_KINDS) {
      hipLaunchKernelGGL(aug_table_kernel, dim3(n_views), blk, 0, s, ops, n_steps, k, npix, hist, lsum, lut);
      MVAL_CHECK_LAUNCH("mval_augment_views/table");
      hipLaunchKernelGGL(aug_apply_kernel, g_bytes, blk, 0, s, img, ops, n_steps, k, nbytes, lut);
      MVAL_CHECK_LAUNCH("mval_augment_views/apply");
    }
    if (kinds & AUG_BIT(MVAL_AUG_COLOR)) {
      hipLaunchKernelGGL(aug_color_kernel, dim3((npix + 1023) / 1024, n_views), blk, 0, s, img, ops, n_steps, k, npix);
      MVAL_CHECK_LAUNCH("mval_augment_views/color");
    }
    if (kinds & AUG_SPATIAL_KINDS) {
      hipLaunchKernelGGL(aug_spatial_kernel, dim3((npix + 255) / 256, n_views), blk, 0, s, img, ops, n_steps, k, h, w, buf);
      MVAL_CHECK_LAUNCH("mval_augment_views/spatial");
      hipLaunchKernelGGL(aug_copy_back_kernel, g_bytes, blk, 0, s, img, ops, n_steps, k, nbytes, buf);
      MVAL_CHECK_LAUNCH("mval_augment_views/copy_back");
    }
  }
  return 0;
}

// ---- uint8 [V][H][W][3] (the reference's channel order) -> float32 [V][3][H][W], normalize_image (utils/triangulation.py:137-145) ----
// The table is pp_lut_kernel's (csrc/preprocess.hip): numpy's float64 expression per byte value and channel, evaluated by the
// workgroup that uses it.  A thread owns 4 pixels; the three planes get one float4 store each where the plane offset allows.
__global__ __launch_bounds__(256) void aug_normalize_kernel(const unsigned char* __restrict__ img, int npix, float* __restrict__ out) {
  __shared__ float lut[3][256];
  {
    const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) lut[ch][threadIdx.x] = (float)(((double)threadIdx.x / 255.0 - mean[ch]) / stdv[ch]);
  }
  __syncthreads();
  const int v = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  if (4 * q >= npix) return;
  const unsigned char* view = img + (int64_t)v * npix * 3;
  unsigned char px[12];
  const int n = aug_load4(view, q, npix, (reinterpret_cast<uintptr_t>(view) & 3) == 0, px);
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    float* o = out + ((int64_t)v * 3 + ch) * npix + 4 * q;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0)
      *reinterpret_cast<float4*>(o) = make_float4(lut[ch][px[ch]], lut[ch][px[3 + ch]], lut[ch][px[6 + ch]], lut[ch][px[9 + ch]]);
    else
      for (int j = 0; j < n; j++) o[j] = lut[ch][px[j * 3 + ch]];
  }
}

extern "C" int mval_normalize_views_u8(const uint8_t* img, int n_views, int h, int w, float* out, void* stream) {
  MVAL_REQUIRE(img && out && n_views > 0 && n_views <= 65535 && h > 0 && w > 0 && (int64_t)h * w * 3 <= (int64_t)1 << 30,
               "mval_normalize_views_u8: bad arguments");
  const int npix = h * w;
  hipLaunchKernelGGL(aug_normalize_kernel, dim3((npix + 1023) / 1024, n_views), dim3(256), 0, mval_stream(stream), img, npix, out);
  MVAL_CHECK_LAUNCH("mval_normalize_views_u8");
  return 0;
}

// ---- the targets: Image.rotate(angle, BICUBIC) on the heat-maps of the views Rotate turned (rotate_targets = "maps") ---------------------
// maps [V][J][H][W] f32, each a Pillow mode-"F" image of its own: ImagingGenericTransform with affine_transform and bicubic_filter32F.  The
// coordinates, the outside test and the taps are those of the uint8 image above; the arithmetic is not: the taps of a row are float32 and
// Geometry.c's BICUBIC forms its coefficient sums from them in float32 (C's float + float), widens, and evaluates the polynomial in float64;
// the four row results are float64 and take aug_cubic as it stands; the result is cast to float32 without a clip (the negative lobes stay).
__device__ __forceinline__ double aug_cubic_f32(float v1, float v2, float v3, float v4, double d) {
  const float p2 = aug_fadd(-v1, v3);
  const float p3 = aug_fadd(aug_fadd(aug_fmul(2.f, aug_fadd(v1, -v2)), v3), -v4);
  const float p4 = aug_fadd(aug_fadd(aug_fadd(-v1, v2), -v3), v4);
  return aug_dadd((double)v2, aug_dmul(d, aug_dadd((double)p2, aug_dmul(d, aug_dadd((double)p3, aug_dmul(d, (double)p4))))));
}

// one thread per output element, maps -> second buffer.  grid (ceil(H * W / 256), J, V) x 256
__global__ __launch_bounds__(256) void aug_rotate_maps_kernel(const float* __restrict__ maps, const mval_aug_op* __restrict__ ops, int n_steps, int step,
                                                              int H, int W, float* __restrict__ out) {
  const int v = blockIdx.z;
  const mval_aug_op* op = ops + (int64_t)v * n_steps + step;
  if (op->kind != MVAL_AUG_ROTATE) return;  // uniform per workgroup
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const int64_t base = ((int64_t)v * gridDim.y + blockIdx.y) * H * W;
  const float* src = maps + base;
  const double xc = x + 0.5, yc = y + 0.5;
  double xin = aug_dadd(aug_dadd(aug_dmul(op->p[0], xc), aug_dmul(op->p[1], yc)), op->p[2]);
  double yin = aug_dadd(aug_dadd(aug_dmul(op->p[3], xc), aug_dmul(op->p[4], yc)), op->p[5]);
  if (!(xin >= 0.0 && yin >= 0.0 && xin < (double)W && yin < (double)H)) {  // outside (or not a number): the fill value
    out[base + i] = 0.f;
    return;
  }
  xin = aug_dadd(xin, -0.5);
  yin = aug_dadd(yin, -0.5);
  const int fx = (int)floor(xin), fy = (int)floor(yin);
  const double dx = aug_dadd(xin, -(double)fx), dy = aug_dadd(yin, -(double)fy);
  int xs[4];
#pragma unroll
  for (int t = 0; t < 4; t++) xs[t] = min(max(fx - 1 + t, 0), W - 1);
  double r[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const float* p = src + (int64_t)min(max(fy - 1 + t, 0), H - 1) * W;
    r[t] = aug_cubic_f32(p[xs[0]], p[xs[1]], p[xs[2]], p[xs[3]], dx);
  }
  out[base + i] = (float)aug_cubic(r[0], r[1], r[2], r[3], dy);
}

// second buffer -> maps for the views of the rotation.  Same grid.
__global__ __launch_bounds__(256) void aug_rotate_maps_copy_back_kernel(float* __restrict__ maps, const mval_aug_op* __restrict__ ops, int n_steps, int step,
                                                                        int npix, const float* __restrict__ buf) {
  const int v = blockIdx.z;
  if (ops[(int64_t)v * n_steps + step].kind != MVAL_AUG_ROTATE) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int64_t e = ((int64_t)v * gridDim.y + blockIdx.y) * npix + i;
  maps[e] = buf[e];
}

// workspace: [V][J][H][W] f32 second buffer
extern "C" size_t mval_rotate_maps_workspace_bytes(int n_views, int maps_per_view, int h, int w) {
  if (n_views <= 0 || maps_per_view <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)n_views * maps_per_view * h * w * sizeof(float);
}

extern "C" int mval_rotate_maps(float* maps, const mval_aug_op* ops, const uint32_t* step_kinds, int n_views, int n_steps, int maps_per_view, int h,
                                int w, void* ws, void* stream) {
  MVAL_REQUIRE(maps && ops && step_kinds && ws && n_views > 0 && n_steps > 0 && maps_per_view > 0 && h > 0 && w > 0, "mval_rotate_maps: bad arguments");
  MVAL_REQUIRE(n_views <= 65535 && maps_per_view <= 65535, "mval_rotate_maps: %d views of %d maps, at most 65535 of either per call", n_views,
               maps_per_view);
  MVAL_REQUIRE((int64_t)h * w <= (int64_t)1 << 28, "mval_rotate_maps: a %d x %d map is too large (at most 2^28 elements)", h, w);
  hipStream_t s = mval_stream(stream);
  const int npix = h * w;
  float* buf = reinterpret_cast<float*>(ws);
  const dim3 blk(256), grid((npix + 255) / 256, maps_per_view, n_views);
  for (int k = 0; k < n_steps; k++) {
    if (!(step_kinds[k] & AUG_BIT(MVAL_AUG_ROTATE))) continue;
    hipLaunchKernelGGL(aug_rotate_maps_kernel, grid, blk, 0, s, maps, ops, n_steps, k, h, w, buf);
    MVAL_CHECK_LAUNCH("mval_rotate_maps/rotate");
    hipLaunchKernelGGL(aug_rotate_maps_copy_back_kernel, grid, blk, 0, s, maps, ops, n_steps, k, npix, buf);
    MVAL_CHECK_LAUNCH("mval_rotate_maps/copy_back");
  }
  return 0;
}
