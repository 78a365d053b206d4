// pixel_convert.h -- a frame of any accepted pixel type as 8-bit RGB on the host, by the rules the GPU kernels apply
// (../hip/pixel_rules.hpp, included by both sides): polychase_core.frame_channel_bytes and the frames of write_images.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../hip/pixel_rules.hpp"

// bytes of one channel of pc_pixel_type `pixel_type`
inline size_t PixelTypeBytes(int pixel_type) { return static_cast<size_t>(pc::pixel_type_bytes(pixel_type)); }

// fp32 pattern of channel c of pixel x in a row of `pixel_type` PC_PIXEL_F16 / PC_PIXEL_F32 (a half widened exactly)
inline uint32_t FloatChannelBits(const uint8_t* row, size_t index, int pixel_type) {
    if (pixel_type == pc::PIXEL_F16) {
        uint16_t h;
        std::memcpy(&h, row + 2 * index, sizeof h);
        return pc::f16_bits_to_f32_bits(h);
    }
    uint32_t b;
    std::memcpy(&b, row + 4 * index, sizeof b);
    return b;
}

// out: rows x cols x 3 bytes, tightly packed: what the default conversion makes of every channel (alpha dropped)
inline void FrameChannelBytes(const uint8_t* data, int rows, int cols, int channels, int pixel_type, size_t row_pitch, uint8_t* out) {
    for (int y = 0; y < rows; y++) {
        const uint8_t* row = data + static_cast<size_t>(y) * row_pitch;
        uint8_t* o = out + static_cast<size_t>(y) * cols * 3;
        for (int x = 0; x < cols; x++)
            for (int c = 0; c < 3; c++) {
                const size_t i = static_cast<size_t>(x) * channels + c;
                uint32_t b;
                if (pixel_type == pc::PIXEL_U8) {
                    b = row[i];
                } else if (pixel_type == pc::PIXEL_U16) {
                    uint16_t v;
                    std::memcpy(&v, row + 2 * i, sizeof v);
                    b = pc::u16_to_u8(v);
                } else {
                    b = pc::f32_bits_to_u8(FloatChannelBits(row, i, pixel_type));
                }
                o[3 * x + c] = static_cast<uint8_t>(b);
            }
    }
}
