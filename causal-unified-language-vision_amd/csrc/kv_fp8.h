// The FP8 KV cache's number format (INTEGRATION.md "FP8 KV cache"), shared by the append /
// dequantise kernels (kv_fp8.hip) and decode attention (decode.hip): OCP e4m3fn codes (gfx950's
// v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8, not the fnuz format of gfx942) with one power-of-two scale
// per token and head, stored as e + 127 in a byte.
#pragma once
#include "common.h"

// e + 127 for a head row whose max |x| is amax (finite, >= 0): e is the smallest integer with
// amax * 2^-e <= 448 = 1.75 * 2^8, from amax's f32 exponent field and mantissa, clamped to e >= -100
// (an all-zero or denormal row: e = -100, codes 0)
DEV int fp8_exp_byte(float amax) {
  const unsigned u = __float_as_uint(amax);
  const int ef = (int)(u >> 23), mant = (int)(u & 0x7FFFFFu);
  return max(ef - 8 + (mant > 0x600000 ? 1 : 0), 27);
}
// 2^e and 2^-e of an exponent byte (27 <= eb <= 247: both normal)
DEV float fp8_scale(int eb) { return __uint_as_float((unsigned)eb << 23); }
DEV float fp8_inv_scale(int eb) { return __uint_as_float((unsigned)(254 - eb) << 23); }

// one value's code (x already scaled: |x| <= 448) and a code's f32 value
DEV unsigned fp8_code(float x) { return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x, 0.f, 0, false) & 0xFFu; }
DEV float fp8_value(unsigned code) { return __builtin_amdgcn_cvt_f32_fp8((int)code, 0); }

// 8 scaled values to 8 codes (8 bytes), and back
DEV u32x2 fp8_pack8(const float* x) {
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0], x[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2], x[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4], x[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6], x[7], hi, true);
  return u32x2{(unsigned)lo, (unsigned)hi};
}
DEV void fp8_unpack4(unsigned w, float* x) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  x[0] = a[0];
  x[1] = a[1];
  x[2] = b[0];
  x[3] = b[1];
}
