// pixel_rules.hpp -- how a channel of a frame's pixel type becomes the byte the gray conversion works on.  One statement of the
// rules for the device kernels (kernels_pyramid.hip, kernels_image.hip) and the host (csrc/host/pixel_convert.h); restated in
// numpy in tests/ingest16_ref.py.  Integers only, except for the one fp32 product of the float rule.
//
//   uint8            the byte itself
//   uint16           the integer nearest to v / 257 (no ties: 257 is odd), so that 257 k -> k for every byte k
//   float16          widened exactly to float32, then the float32 rule
//   float32          numpy `(x * 255).astype(uint8)`: truncate toward zero, the low byte; out of int32 range and NaN -> 0
//                    (or, under a float transfer table, the table's entry at transfer_index of the bits: common.hpp)
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define PC_RULE_FN __host__ __device__ __forceinline__
#else
#define PC_RULE_FN inline
#endif

namespace pc {

// == pc_pixel_type of include/polychase_hip.h
enum PixelType { PIXEL_U8 = 0, PIXEL_U16 = 1, PIXEL_F16 = 2, PIXEL_F32 = 3 };
PC_RULE_FN int pixel_type_bytes(int pixel_type) { return pixel_type == PIXEL_F32 ? 4 : (pixel_type == PIXEL_U8 ? 1 : 2); }

// (2 v + 257) / 514 rounded down = round(v / 257), as one multiply and a shift: 255 / 65535 = 1 / 257, 32895 = 2^15 + 127
PC_RULE_FN uint32_t u16_to_u8(uint32_t v) { return (v * 255u + 32895u) >> 16; }

// IEEE binary16 pattern -> the binary32 pattern of the same value: every half is a float (subnormals become normal numbers,
// +-0 and +-inf keep their sign, a NaN keeps sign and payload)
PC_RULE_FN uint32_t f16_bits_to_f32_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 31u;
    uint32_t m = h & 0x3ffu;
    if (e == 0u) {
        if (m == 0u) return sign;
        // m * 2^-24: shift the leading one to bit 10 (s = 1 .. 10), the exponent falls by as much from 2^-14
        const uint32_t s = (uint32_t)__builtin_clz(m) - 21u;
        m = (m << s) & 0x3ffu;
        return sign | ((113u - s) << 23) | (m << 13);
    }
    if (e == 31u) return sign | 0x7f800000u | (m << 13);
    return sign | ((e + 112u) << 23) | (m << 13);
}

// the float32 rule without a table; `bits` is the channel's fp32 pattern
PC_RULE_FN uint32_t f32_bits_to_u8(uint32_t bits) {
    float v;
    __builtin_memcpy(&v, &bits, sizeof v);
    const float s = v * 255.0f;
    const int i = (s >= -2147483648.0f && s < 2147483648.0f) ? (int)s : (int)0x80000000;
    return (uint32_t)i & 0xffu;
}

}  // namespace pc
