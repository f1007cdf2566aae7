// "P2" activations: every fp32 activation value kept as the PAIR of fp16 planes the fp16x2-split MFMA convs consume,
// written once by the producer's epilogue (csrc/conv_p2.hip, conv_block_p2.hip).
//
//   tensor of N images, C channels (C % 8 == 0), H x W:
//       halves  [n][plane p = 0 (h), 1 (l)][C / 8][H][W][8]          4 bytes per element, like fp32
//       x[n][c][y][x] = (h + l) * 2^-s[n]         h = RNE_fp16(x * 2^s), l = RNE_fp16(x * 2^s - h)
//   row of the tensor's image n (P2_ROW = 512 dwords; the fp32-activation kernels' rows are MVAL_AMAX_ROW = 4096):
//       row[0 .. P2_SLOTS - 1] = partial max |x| (float bits; one slot per producing workgroup, unused slots stay 0:
//                                the rows are zeroed once when the plan is built and a slot only ever belongs to one
//                                workgroup, so a consumer reads a FIXED number of slots -- no count, no dependent load),
//       row[P2_INV_SLOT] = float bits of 2^-s[n]
//
// Why: with fp32 NHWC activations every CONSUMER re-splits each element it stages (12 vector instructions per
// float4, two 8-byte LDS stores) -- 2.4x per element for a 3x3 conv's halo and once more per cout group.  With
// P2 the consumer's staging is a 16-byte copy (global -> register -> LDS, no arithmetic), and the channel-blocked
// layout makes the LDS image [8-channel block][pixel][16 B] conflict-free for ds_read_b128 at ANY pixel offset
// (a 16-lane fragment read covers 256 consecutive bytes per block), so the 3x3 taps are plain immediate offsets.
//
// The scale 2^s[n] must be known BEFORE the producer's first store, i.e. before the image's true maximum exists.
// It comes from a rigorous per-image bound of the fused operator out = act((bn(conv(x)) + r1) + r2):
//       |out| <= A * max|x| + B + max|r1| + max|r2|,   A = max_c |scale_c| * sum_k |w_ck|,  B = max_c |shift_c|
// (A, B per layer at parameter-refresh time; the maxima are the exact per-image maxima the producers keep).  The
// bound is typically 2^4 .. 2^7 above the true maximum; fp16's 5 exponent bits absorb that: 2^s puts the BOUND in
// [2^13, 2^14), every value above 2^-3 (scaled) keeps all 22 significand bits of the pair and smaller ones an
// absolute error <= 2^-25, i.e. <= 2^-38 of the bound.  Per IMAGE, so results do not depend on the batch.
#pragma once
#include "conv_common.h"

#define P2_ROW 512    // dwords per (tensor, image) row
#define P2_SLOTS 256  // partial maxima per image: 4 per lane of the reading wave
#define P2_INV_SLOT (P2_ROW - 1)

typedef _Float16 p2_f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 p2_f16x8 __attribute__((ext_vector_type(8)));
typedef float p2_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int p2_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int p2_u32x2 __attribute__((ext_vector_type(2)));
// the short names the P2 units use (the same types as the other conv units' own typedefs of these names)
typedef p2_f32x4 f32x4;
typedef p2_f16x8 f16x8;
typedef p2_f16x4 f16x4;
typedef p2_u32x4 u32x4;
typedef p2_u32x2 u32x2;

// s_setprio of a wave's vector phases (epilogues, BN + split between two convs): they win issue arbitration against the partner wave's
// MFMA stream (round 3) ...
constexpr int P2_VALU_PRIO = 2;
// ... and around every step's MFMA group of conv_p2.hip / conv_block_p2.hip: 2.98-3.09 -> 2.57-2.62 us per stage of the loop's
// skeleton (profiles/r06/p2_loop_order_prefetch.log)
constexpr int P2_MFMA_PRIO = 1;

__device__ __forceinline__ p2_f32x4 p2_mfma(const p2_u32x4 a, const p2_u32x4 b, const p2_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(p2_f16x8, a), __builtin_bit_cast(p2_f16x8, b), c, 0, 0, 0);
}

// 2^s that puts `bound` in [2^13, 2^14) and its inverse (zero / inf / NaN bound: unscaled)
__device__ __forceinline__ void p2_scale_of(float bound, float& mul, float& inv) {
  const int e = (int)((__float_as_uint(bound) >> 23) & 0xff);
  int s = (e == 0 || e == 255) ? 0 : 13 - (e - 127);
  s = max(-110, min(110, s));
  mul = __uint_as_float((unsigned)(127 + s) << 23);
  inv = __uint_as_float((unsigned)(127 - s) << 23);
}

// max(v, floor) that PROPAGATES NaN (IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950), for the ReLU / "no activation"
// clamps of the epilogues: fmaxf returns the other operand for a NaN, which turned a diverged model's NaNs into 0 (ReLU) or
// -inf where torch -- and the h2 / bf3 / fp32 plans -- hand them on.
__device__ __forceinline__ float p2_max_nan(float v, float floor_) { return __builtin_elementwise_maximum(v, floor_); }

__device__ __forceinline__ void p2_split(const p2_f32x4 v, p2_f16x4& h, p2_f16x4& l) {
  h = __builtin_convertvector(v, p2_f16x4);
  // v - float(h) as ONE v_fma_mix_f32 per value (fma(float(h), -1, v): the same singly-rounded difference as convert +
  // subtract; the compiler does not form it by itself): 8 instead of 12 instructions per split
  const p2_u32x2 hu = __builtin_bit_cast(p2_u32x2, h);
  p2_f32x4 r;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r.x) : "v"(hu.x), "v"(v.x));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.y) : "v"(hu.x), "v"(v.y));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r.z) : "v"(hu.y), "v"(v.z));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r.w) : "v"(hu.y), "v"(v.w));
  l = __builtin_convertvector(r, p2_f16x4);
}
__device__ __forceinline__ p2_f32x4 p2_join(const p2_f16x4 h, const p2_f16x4 l) {
  // float(h) * 1 + float(l), exact (22 bits), in one v_fma_mix_f32 per value (both operands read as fp16 halves): 4 instead of 12
  const p2_u32x2 hu = __builtin_bit_cast(p2_u32x2, h), lu = __builtin_bit_cast(p2_u32x2, l);
  p2_f32x4 r;
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r.x) : "v"(hu.x), "v"(lu.x));
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r.y) : "v"(hu.x), "v"(lu.x));
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r.z) : "v"(hu.y), "v"(lu.y));
  asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r.w) : "v"(hu.y), "v"(lu.y));
  return r;
}

// A workgroup's max |x| of what it stored of image n -> its slot of the row.  More producing workgroups per image than
// slots (inputs above ~512 x 512): they fold into slot % P2_SLOTS with atomicMax (the launcher zeroes the rows first).
__device__ __forceinline__ void p2_slot_put(unsigned* row, int slot, int total, unsigned bits) {
  if (total <= P2_SLOTS) row[slot] = bits;
  else atomicMax(row + slot % P2_SLOTS, bits);
}
// Consumer side: the lanes' share of the partial slots of image n (4 independent loads) ...
struct P2RowRegs {
  unsigned v[P2_SLOTS / 64];
  unsigned inv;
};
__device__ __forceinline__ void p2_row_request(const unsigned* rows, int n, P2RowRegs& r) {
  const unsigned* row = rows + (int64_t)n * P2_ROW;
#pragma unroll
  for (int i = 0; i < P2_SLOTS / 64; i++) r.v[i] = row[i * 64 + (threadIdx.x & 63)];
  r.inv = row[P2_INV_SLOT];
}
// Maximum over the wave of non-negative float bits (they order like unsigned integers), uniform result: four DPP
// steps inside the 16-lane rows, then the four rows through scalar registers -- a dozen instructions; the
// __shfl_xor butterfly is six dependent ds_bpermute round trips (~0.3 us each time it is used in an epilogue).
__device__ __forceinline__ unsigned p2_wave_umax(unsigned m) {
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xf, 0xf, false));  // row_half_mirror
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xf, 0xf, false));  // row_mirror
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)m, 0), b = (unsigned)__builtin_amdgcn_readlane((int)m, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)m, 32), d = (unsigned)__builtin_amdgcn_readlane((int)m, 48);
  return max(max(a, b), max(c, d));
}
// Sum over each 16-lane row of the wave, in every lane of the row (four DPP steps, fixed order: deterministic)
__device__ __forceinline__ float p2_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));  // row_mirror
  return v;
}
// Maximum over each 16-lane row of the wave, in every lane of the row
__device__ __forceinline__ float p2_row16_max(float v) {
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false)));
  return v;
}
// ... and their maximum (uniform over the wave)
__device__ __forceinline__ float p2_row_amax(const P2RowRegs& r) {
  unsigned m = r.v[0];
#pragma unroll
  for (int i = 1; i < P2_SLOTS / 64; i++) m = max(m, r.v[i]);
  return __uint_as_float(p2_wave_umax(m));
}

// Launcher side of the persistent kernels: resident workgroups per CU of one kernel instantiation, from its LDS size and its
// register count (allocation granule 8, 512 per SIMD lane; hipOccupancyMaxActiveBlocksPerMultiprocessor's answer was not
// usable: with it the 32-channel block kernel ran 20x slower).  `slot` is the instantiation's own static std::atomic<int>
// (0 = not computed yet): threads racing on the first launch compute the same value, so no lock is needed.
#include <atomic>
int mval_cu_count();  // common.hip: compute units of the CURRENT device (hipDeviceProp_t::multiProcessorCount), cached per device
template <typename K>
static inline int p2_resident_wgs(K kernel, std::atomic<int>& slot, size_t smem, int waves_per_wg) {
  int nb = slot.load(std::memory_order_relaxed);
  if (nb) return nb;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipFuncAttributes fa;
  nb = (int)((160 * 1024) / smem);
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess && fa.numRegs > 0) {
    const int waves_simd = 512 / ((fa.numRegs + 7) / 8 * 8);
    nb = min(nb, max(1, waves_simd * 4 / waves_per_wg));
  } else {
    nb = min(nb, 2);
  }
  if (nb < 1) nb = 1;
  slot.store(nb, std::memory_order_relaxed);
  return nb;
}

// ---- the persistent tile walk of conv_p2 / block / bneck / stem --------------------------------------------------------------------
// A launch covers tiles_total = tiles_x * tiles_y * N tiles with wgs_x workgroups per cout group.  Workgroup b belongs to XCD group
// b % 8 (one workgroup: one group), every group owns a contiguous range of `per` tiles -- neighbouring tiles' halos meet in one L2 --
// and its wgs_x / 8 workgroups walk that range in steps of wgs_x / 8.  So a count of 8 or more MUST be a multiple of 8: with 12
// workgroups for 12 tiles the floor wgs_x / 8 = 1 made four tiles run twice -- harmless for stored outputs, wrong for anything a
// kernel accumulates over its walk (the batch-statistics sums of EPI 3).  mval_p2_walk_grid is the one place that decides the count.
struct P2Walk {
  int tiles_x, tiles_y, tiles_total, wgs_x;
  unsigned tiles_img_magic, tiles_x_magic;  // 2^32 / d + 1 (0: d == 1): tile index -> (image, tile row) without a divide, t * d < 2^32
};
static inline void p2_walk_fill(P2Walk& w, int hout, int wout, int th, int tw, int n) {
  w.tiles_x = (wout + tw - 1) / tw;
  w.tiles_y = (hout + th - 1) / th;
  const int tiles_img = w.tiles_x * w.tiles_y;
  w.tiles_total = tiles_img * n;
  w.tiles_img_magic = tiles_img > 1 ? (unsigned)(((uint64_t)1 << 32) / (unsigned)tiles_img + 1) : 0u;
  w.tiles_x_magic = w.tiles_x > 1 ? (unsigned)(((uint64_t)1 << 32) / (unsigned)w.tiles_x + 1) : 0u;
}
// Workgroups per cout group (the grid's x) for `resident` workgroups that fit the device at once, shared by `groups` cout groups: as
// many as stay resident, a multiple of 8; fewer tiles than that: one tile each (8 or more: rounded up to a multiple of 8, the
// workgroups without a tile return at once); more: equal shares, so that no workgroup walks a round more than the others.  (No
// workgroup waits for another one: an optimistic `resident` only costs a second round.)  conv_p2.hip; a C symbol for the host test.
extern "C" int mval_p2_walk_grid(int tiles_total, int resident, int groups);
// this workgroup's first tile, the end of its range and its step
__device__ __forceinline__ void p2_walk_begin(const P2Walk w, int& tile, int& tile_end, int& wgx) {
  const int X = w.wgs_x >= 8 ? 8 : 1;
  const int per = (w.tiles_total + X - 1) / X;
  wgx = w.wgs_x / X;
  const int xg = (int)blockIdx.x % X;
  tile = xg * per + (int)blockIdx.x / X;
  tile_end = min(w.tiles_total, (xg + 1) * per);
}
// tile t -> image, first output row / column of its TH x TW pixels (tiles_img = w.tiles_x * w.tiles_y: every caller keeps it anyway)
template <int TH, int TW>
__device__ __forceinline__ void p2_walk_decode(const P2Walk w, const int tiles_img, int t, int& n, int& oy0, int& ox0) {
  n = w.tiles_img_magic ? (int)__umulhi((unsigned)t, w.tiles_img_magic) : t;
  const int r = t - n * tiles_img;
  const int tyi = w.tiles_x_magic ? (int)__umulhi((unsigned)r, w.tiles_x_magic) : r;
  oy0 = tyi * TH;
  ox0 = (r - tyi * w.tiles_x) * TW;
}

// ---- diagnostic builds (-DP2_STAMP) of the fused kernels: eight phase timers per wave from the 100 MHz wall clock, left in
// a.dbg[workgroup * 4 + wave][16] = [start, start, -, -, end, -, -, -, timers] (tools/p2_block_stamps.py, p2_bneck_stamps.py,
// p2_stem_stamps.py).  P2F_T0 starts, P2F_ACC(k) adds the time since the last P2F_T0 / P2F_ACC to timer k, P2F_FLUSH stores.
#ifdef P2_STAMP
#define P2F_T0 unsigned long long bp_t = wall_clock64(), bp_t00 = bp_t; unsigned long long bp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define P2F_ACC(k)                                \
  do {                                            \
    const unsigned long long t_ = wall_clock64(); \
    bp_acc[k] += t_ - bp_t;                       \
    bp_t = t_;                                    \
  } while (0)
#define P2F_FLUSH                                                                                    \
  do {                                                                                               \
    if (a.dbg && lane == 0) {                                                                        \
      unsigned long long* d_ = a.dbg + ((int64_t)blockIdx.x * 4 + wave) * 16;                        \
      d_[0] = bp_t00; d_[4] = wall_clock64(); d_[1] = d_[0];                                         \
      for (int k_ = 0; k_ < 8; k_++) d_[8 + k_] = bp_acc[k_];                                        \
    }                                                                                                \
  } while (0)
extern unsigned long long* g_p2_dbg_shared;  // conv_p2.hip: the buffer mval_p2_debug_buffer() registered
#else
#define P2F_T0
#define P2F_ACC(k)
#define P2F_FLUSH
#endif

struct P2Args {
  const _Float16* in;  // P2 planes of the input tensor
  const float* w;      // MVAL_PACK_MFMA16_H2 fragments (+ trailer)
  const float* w_unscale;
  const float* scale;
  const float* shift;
  const float* bound;  // [A, B]
  const _Float16* res1;
  const _Float16* res2;
  const unsigned* in_row;
  const unsigned* res1_row;
  const unsigned* res2_row;
  unsigned* out_row;
  _Float16* out;    // P2 planes ...
  float* out_f32;   // ... or fp32 NCHW (the heat-map layer)
  // ... or (training forward, round 4: EPI 3) the RAW conv output z = acc * 2^-s as fp32 NHWC, for train-mode BatchNorm; bn_part != nullptr:
  // every (workgroup, pixel-wave) also leaves the per-channel (sum, sum of squares) of what it stored over its whole tile walk,
  // float64 [cout][bn_slots][2] (bn_slots = wgs_x * WM, filled by the launcher and reported in *bn_slots_host)
  float* out_nhwc;
  int acc_nhwc;  // (EPI 3) != 0: out_nhwc += the result instead of = (a data gradient accumulating into the producer's gradient slot)
  double* bn_part;
  int64_t bn_part_cap;
  int* bn_slots_host;
  int bn_slots;
  unsigned long long* argmax_keys;  // heat-map layer: != nullptr = also keep the arg-max keys of every map, [N][MVAL_ARGMAX_SLOTS][Cout] (mval_common.h)
  int N, Hin, Win, Cin, Hout, Wout, Cout;  // Hout / Wout before the fused upsample
  int k, stride;
  int up, relu;
  // (round 5) k == 2: one PARITY of a transposed conv / of a stride-2 conv's data gradient (four 2 x 2 stride-1 convs over the input grid,
  // conv_mfma_split.hip's pack modes 3 / 4): the window of output pixel (y, x) covers input rows y - pad_y .. y - pad_y + 1 (pad_y = 1 - py;
  // columns alike), Hout x Wout = the INPUT grid, and with os = 1 the result goes to pixel (2 y + oy, 2 x + ox) of a (2 Hout) x (2 Wout)
  // tensor (P2 planes or the fp32 NHWC slot).  The four launches of a tensor share its rows: slot_base / slot_total give each its share
  // of the partial-maximum slots, keep_rows != 0 stops the launcher from zeroing rows an earlier parity has already written.
  int pad_y, pad_x, os, oy, ox, slot_base, slot_total, keep_rows;
  // in_sub = 1 (k == 1): the conv reads every second pixel of its input (a stride-2 1 x 1 conv as a stride-1 one over the sub-sampled view:
  // pose_resnet.py's downsample branches); Hin / Win stay the full input size, Hout / Wout = ceil(Hin / 2), ceil(Win / 2)
  int in_sub;
  int th, tw;
  P2Walk walk;  // tiles of th x tw output pixels
  int NS_total;
  int amax_tiles;
  unsigned long long* dbg;  // diagnostic builds (-DP2_STAMP): per-wave phase time stamps; nullptr otherwise
  // (round 6, training forward, EPI 3, 3x3 stride 1) in_z != nullptr: the input activation does not exist as planes -- it is
  // relu(BatchNorm(in_z)) of the producer's RAW conv output in_z (fp32 NHWC, N x Hin x Win x Cin) with the producer's batch statistics and
  // affine parameters, and the staging applies it while it copies: the same alpha = invstd * gamma, beta' = fma(-mean, alpha, beta),
  // r = fma(z, alpha, beta'), ReLU, scale 2^s from Samuelson's bound max_c(|gamma| sqrt(M - 1) + |beta|), split into (h, l) as the separate
  // apply pass (train_ops.hip bn_apply_fwd_p2_kernel) writes -- the LDS image is bit-identical to the one staged from its planes.
  const float* in_z;
  const float* zin_mean; const float* zin_invstd; const float* zin_gamma; const float* zin_beta;
  float zin_sqrt_m1;
  // (round 6, a data gradient, EPI 3) bs_z != nullptr: the tensor this launch writes is the gradient g of relu(BatchNorm(bs_z)) and this
  // launch is its ONLY writer -- the epilogue also leaves what the BatchNorm backward's reduction pass would compute from a second read of
  // it: per (workgroup, pixel wave) slot and channel the sums of m g and m g xhat (m = BatchNorm(z) > 0, xhat = (z - mean) invstd; float64
  // bs_part[slot][Cout][2]) and max |m g| (float bs_gmax[slot][Cout], behind the sums); *bs_slots_host = the number of slots (0: no room
  // in bs_cap doubles -- nothing kept).  bs_bound_slot: the dword the reduction pass zeroes for its finalize kernel.
  const float* bs_z;
  const unsigned char* bs_mask;  // != nullptr: m comes from the (out > 0) bits the producer's forward apply kept (one byte per float4: a ReLU behind
                                 // residual adds, train_ops.hip mask mode 3) and this launch may ACCUMULATE (acc_nhwc): it is the slot's LAST writer
  const float* bs_mean; const float* bs_invstd; const float* bs_gamma; const float* bs_beta;
  double* bs_part;
  float* bs_gmax;
  int64_t bs_cap;
  int* bs_slots_host;
  int bs_slots;
  unsigned* bs_bound_slot;
};

int mval_launch_conv_p2(const P2Args& a, hipStream_t s);  // conv_p2.hip; 1 = unsupported (dry != 0: no launch)
int mval_conv_p2_form_of(const P2Args& a, mval_p2_form* form);  // 1 + the form the launcher would run, 0 if unsupported; no launch, no HIP call
// the geometry of a conv of the training forward on these kernels and of its data gradient (net_train.hip; net.hip mval_conv_p2_form)
static inline void p2_train_fwd_geometry(P2Args& p, const mval_op& op, int n_images) {
  p.N = n_images; p.Hin = op.hin; p.Win = op.win; p.Cin = op.cin; p.Hout = op.hout; p.Wout = op.wout; p.Cout = op.cout;
  p.k = op.k; p.stride = op.stride;
}
static inline void p2_dgrad_geometry(P2Args& p, const mval_op& op, int n_images) {
  p.N = n_images; p.Hin = op.hout; p.Win = op.wout; p.Cin = op.cout; p.Hout = op.hin; p.Wout = op.win; p.Cout = op.cin;
  p.k = op.k; p.stride = 1;
}
int mval_launch_nhwc_to_p2(const float* x, const unsigned* rows_in, _Float16* planes, unsigned* rows, int n_images, int HW, int C,
                            hipStream_t s);
int mval_conv_p2_supported(int k, int stride, int cin, int cout, int hin, int win, int up, int out_nchw, int n);
int mval_conv_p2_inz_supported(int cin, int cout, int h, int w, int n);  // the in_z form above (3x3 stride 1, raw fp32 NHWC out)
int mval_conv_p2_bsum_supported(int cin, int cout, int h, int w, int n);  // the bs_z form (3x3 stride-1 data gradient: cin = the conv's cout)
int mval_conv_p2_parity_supported(int cin, int cout, int h, int w, int n, int nhwc_out);  // one parity conv (k 2) over an h x w grid

// conv_block_p2.hip: a whole BasicBlock over P2 activations in one launch; 1 = unsupported
int mval_conv_block_p2_supported(int C, int N, int H, int W);
int mval_launch_conv_block_p2(int C, const void* in, void* out, const float* w1, const float* w1_unscale, const float* scale1,
                              const float* shift1, const float* bound1, const float* w2, const float* w2_unscale, const float* scale2,
                              const float* shift2, const float* bound2, const unsigned* in_row, unsigned* out_row, int N, int H, int W,
                              hipStream_t s);
// conv_bneck_p2.hip: a whole Bottleneck (cin -> 64 -> 64 -> 256, cin = 64 or 256) over P2 activations in one launch; the
// arrays hold the FLOAT OFFSETS into `params` of conv1 / conv2 / conv3's packed weights, their trailers, BN vectors and
// bounds; 1 = unsupported
int mval_conv_bneck_p2_supported(int cin, int planes, int N, int H, int W);
int mval_launch_conv_bneck_p2(int cin, const void* in, const void* res, void* out, const float* params, const int64_t* w, const int64_t* w_unscale,
                              const int64_t* scale, const int64_t* shift, const int64_t* bound, const unsigned* in_row,
                              const unsigned* res_row, unsigned* out_row, int N, int H, int W, hipStream_t s);
// conv_stem_p2.hip: HRNet's stem (3 -> 64 -> 64 channels, two 3x3 stride-2 convs) from the fp32 NCHW image to P2 planes in
// one launch (plus a small max |x| pass over the image into in_row); 1 = unsupported
int mval_conv_stem_p2_supported(int N, int H, int W);
int mval_launch_conv_stem_p2(const float* in, void* out, const float* w1, const float* scale1, const float* shift1, const float* bound1,
                             const float* w2, const float* w2_unscale, const float* scale2, const float* shift2, const float* bound2,
                             unsigned* in_row, unsigned* out_row, int N, int H, int W, hipStream_t s);
// conv_fuse_up_p2.hip: the two or three up-sampling 1x1 terms of a fuse-layer output (32 / 64 channels) added to the partial
// sum `res` in one launch; arrays per term (float offsets into `params`); 1 = unsupported
int mval_conv_fuse_up_p2_supported(int cout, int n_terms, const int* cin, const int* up, int N, int H, int W);
int mval_launch_conv_fuse_up_p2(int cout, int n_terms, int relu, const void* res, const unsigned* res_row, void* out, unsigned* out_row, const float* params,
                                const void* const* in, const unsigned* const* in_row, const int* cin, const int* up, const int64_t* w,
                                const int64_t* w_unscale, const int64_t* scale, const int64_t* shift, const int64_t* bound, int N, int H, int W,
                                hipStream_t s);
