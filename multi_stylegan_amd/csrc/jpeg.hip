// Baseline JPEG (ITU T.81, sequential DCT, Huffman, 8 bit), 4:2:0, from the interleaved RGB bytes msg_sample_sheet writes to
// the entropy-coded scan of every frame of a batch: what a Motion-JPEG file needs of the device.  The host adds the headers
// (multi_stylegan_amd/video.py: jpeg_file, MjpegWriter).  The arithmetic is fixed in include/msg_hip.h.
//
// Four launches on the caller's stream, no synchronisation, nothing read back:
//   1 jpeg_transform_kernel  one workgroup (192 lanes) per 4 MCUs: the 16 x 64 pixel tile goes to LDS once (dword loads where a
//                            row is 4-byte aligned and inside the picture, clamped byte loads at the edges), a lane owns one
//                            row of one of the 24 blocks for the row pass and one column for the column pass (LDS in between),
//                            quantises, and the zigzag blocks leave as 16-byte stores -> coefficients [N, MR, MC, 6, 64] in ws
//                            (and in `coef` where the caller wants them)
//   2 jpeg_interval_kernel   one workgroup (256 lanes) per restart interval (one MCU row of one frame).  The interval is walked
//                            in chunks of 256 blocks, a lane per block: the lane codes its block's (run, size) symbols from the
//                            block's nonzero mask, once to count bits and -- after a workgroup scan of the counts -- once to OR
//                            them into the chunk's bit buffer in LDS (atomicOr on 32-bit LDS words: the result does not depend
//                            on the order).  Whole bytes then leave for the interval's slot of the staging area with FF -> FF 00
//                            (a second scan, over the FF counts); up to seven bits carry into the next chunk.  So LDS bounds the
//                            chunk, not the width.  The interval's byte count goes to ws.
//   3 jpeg_offsets_kernel    one workgroup: exclusive prefix sum of the N * MR byte counts, offsets[0 .. N]
//   4 jpeg_pack_kernel       one workgroup per interval: staging slot -> its dense place in `scan`
// No chain runs over the blocks of a frame: DC prediction reads the neighbouring block's DC from the coefficient array.
#include "msg_common.h"

namespace {

constexpr int JPEG_GROUP = 4;                        // MCUs per workgroup of the transform
constexpr int JPEG_CHUNK = 256;                      // blocks per chunk of the interval coder: one per lane
// the most bits one block can code to: DC 11 (code) + 11, 63 x (16 (code) + 10) = 1660 -> 52 words
constexpr int JPEG_BLOCK_WORDS = 52;
constexpr int JPEG_BLOCK_BYTES = 4 * JPEG_BLOCK_WORDS;
constexpr int JPEG_BUF_WORDS = JPEG_CHUNK * JPEG_BLOCK_WORDS + 2;

// entry = length << 16 | code; index: the symbol (DC: the size category; AC: run << 4 | size)
struct JpegHuff {
    unsigned int dc[2][12];
    unsigned int ac[2][256];
};

struct JpegSpec {
    unsigned char bits[16];
    unsigned char vals[162];
};

// T.81 Annex K.3.3: tables K.3 - K.6 as BITS / HUFFVAL
constexpr JpegSpec JPEG_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegSpec JPEG_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr JpegSpec JPEG_AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr JpegSpec JPEG_AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// T.81 Annex C: codes of one length are consecutive, the first of a length is twice the one past the last of the length before
constexpr void jpeg_fill(unsigned int* table, const JpegSpec& spec) {
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < spec.bits[len - 1]; ++i) table[spec.vals[k++]] = ((unsigned int)len << 16) | code++;
        code <<= 1;
    }
}

constexpr JpegHuff jpeg_make_huff() {
    JpegHuff h = {};
    jpeg_fill(h.dc[0], JPEG_DC_LUMA);
    jpeg_fill(h.dc[1], JPEG_DC_CHROMA);
    jpeg_fill(h.ac[0], JPEG_AC_LUMA);
    jpeg_fill(h.ac[1], JPEG_AC_CHROMA);
    return h;
}

struct JpegZigzag {
    unsigned char of_natural[64];                    // natural (row-major) index -> position in the zigzag sequence
};

constexpr JpegZigzag jpeg_make_zigzag() {            // T.81 figure A.6, walked
    JpegZigzag z = {};
    int r = 0, c = 0;
    for (int k = 0; k < 64; ++k) {
        z.of_natural[r * 8 + c] = (unsigned char)k;
        if ((r + c) % 2 == 0) {                      // moving up and to the right
            if (c == 7) ++r; else if (r == 0) ++c; else { --r; ++c; }
        } else {
            if (r == 7) ++c; else if (c == 0) ++r; else { ++r; --c; }
        }
    }
    return z;
}

__constant__ JpegHuff jpeg_huff = jpeg_make_huff();
__constant__ JpegZigzag jpeg_zigzag = jpeg_make_zigzag();

struct JpegQuant {
    unsigned short q[128];                           // luma then chroma, natural order: a kernel argument, validated on the host
};

// X[u] = C(u) / 2 sum_j x[j] cos((2 j + 1) u pi / 16), C(0) = 1 / sqrt 2: T.81 A.3.3 in one dimension, as the sums and
// differences of mirrored samples (even u see x[j] + x[7 - j], odd u see x[j] - x[7 - j])
__device__ __forceinline__ void jpeg_dct8(float* x) {
    constexpr float c1 = 0.98078528040323044913f, c2 = 0.92387953251128675613f, c3 = 0.83146961230254523708f;
    constexpr float c4 = 0.70710678118654752440f, c5 = 0.55557023301960222474f, c6 = 0.38268343236508977173f;
    constexpr float c7 = 0.19509032201612826785f;
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
    x[0] = (0.5f * c4) * (e0 + e1);
    x[4] = (0.5f * c4) * (e0 - e1);
    x[2] = 0.5f * (c2 * e2 + c6 * e3);
    x[6] = 0.5f * (c6 * e2 - c2 * e3);
    x[1] = 0.5f * (c1 * d0 + c3 * d1 + c5 * d2 + c7 * d3);
    x[3] = 0.5f * (c3 * d0 - c7 * d1 - c1 * d2 - c5 * d3);
    x[5] = 0.5f * (c5 * d0 - c1 * d1 + c7 * d2 + c3 * d3);
    x[7] = 0.5f * (c7 * d0 - c5 * d1 + c3 * d2 - c1 * d3);
}

// grid (ceil(MC / 4), MR, N), 192 lanes: lane = (MCU m of 4, block k of 6, row / column r of 8)
__global__ __launch_bounds__(192) void jpeg_transform_kernel(const unsigned char* __restrict__ rgb, JpegQuant quant,
                                                             short* __restrict__ coef_ws, short* __restrict__ coef, int H, int W,
                                                             int MR, int MC) {
    __shared__ unsigned int tile[16][48];                                    // 16 rows x 64 pixels x 3 bytes
    __shared__ float pass[24][8][9];                                         // row-transformed blocks (rows padded to 9)
    __shared__ __attribute__((aligned(16))) short zz[24 * 64];               // quantised, zigzag
    const int tid = threadIdx.x;
    const int mc0 = blockIdx.x * JPEG_GROUP, mr = blockIdx.y, n = blockIdx.z;
    const int x0 = mc0 * 16, y0 = mr * 16;
    const bool inside = x0 + 16 * JPEG_GROUP <= W;
    for (int i = tid; i < 16 * 48; i += 192) {
        const int row = i / 48, w = i - row * 48;
        const int y = min(y0 + row, H - 1);                                  // rows below the picture repeat the last one
        const unsigned char* line = rgb + ((long long)n * H + y) * W * 3;
        unsigned int v;
        if (inside && (((uintptr_t)(line + 3ll * x0)) & 3u) == 0) {
            v = *reinterpret_cast<const unsigned int*>(line + 3ll * x0 + 4 * w);
        } else {
            v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int byte = 4 * w + k, px = byte / 3, ch = byte - 3 * px;
                const int x = min(x0 + px, W - 1);                           // columns right of the picture repeat the last one
                v |= (unsigned int)line[3ll * x + ch] << (8 * k);
            }
        }
        tile[row][w] = v;
    }
    __syncthreads();

    const unsigned char* px = reinterpret_cast<const unsigned char*>(&tile[0][0]);
    const int block = tid >> 3, r = tid & 7;                                 // block = 6 m + k
    const int m = block / 6, k = block - 6 * m;
    float x[8];
    if (k < 4) {
        const unsigned char* p = px + ((k >> 1) * 8 + r) * 192 + (m * 16 + (k & 1) * 8) * 3;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            x[j] = 0.299f * p[3 * j] + 0.587f * p[3 * j + 1] + 0.114f * p[3 * j + 2] - 128.0f;
    } else {
        // (the + 128 of Cb / Cr and the level shift cancel)
        const float cr = k == 4 ? -0.168736f : 0.5f, cg = k == 4 ? -0.331264f : -0.418688f, cb = k == 4 ? 0.5f : -0.081312f;
        const unsigned char* p = px + (2 * r) * 192 + (m * 16) * 3;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float sum = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const unsigned char* q = p + dy * 192 + (2 * j + dx) * 3;
                    sum += cr * q[0] + cg * q[1] + cb * q[2];
                }
            x[j] = 0.25f * sum;
        }
    }
    jpeg_dct8(x);
#pragma unroll
    for (int j = 0; j < 8; ++j) pass[block][r][j] = x[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = pass[block][j][r];                    // column r: horizontal frequency r
    jpeg_dct8(x);
    const unsigned short* qt = quant.q + (k < 4 ? 0 : 64);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int natural = v * 8 + r;
        float mag = floorf(fabsf(x[v]) / (float)qt[natural] + 0.5f);
        if (natural != 0) mag = fminf(mag, 1023.0f);                         // the categories the AC tables code
        zz[block * 64 + jpeg_zigzag.of_natural[natural]] = (short)(int)copysignf(mag, x[v]);
    }
    __syncthreads();
    if (mc0 + m < MC) {                                                      // 8 coefficients a lane: lane t holds zz[8 t ..]
        const long long at = ((((long long)n * MR + mr) * MC + mc0) * 6) * 64 + 8ll * tid;
        const uint4 v = *reinterpret_cast<const uint4*>(&zz[8 * tid]);
        *reinterpret_cast<uint4*>(coef_ws + at) = v;
        if (coef) {
            if ((((uintptr_t)coef) & 15u) == 0) {
                *reinterpret_cast<uint4*>(coef + at) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) coef[at + j] = zz[8 * tid + j];
            }
        }
    }
}

// ---- the interval coder
// bit `pos` of the buffer is bit 31 - pos % 32 of word pos / 32: the stream's byte order.  len <= 27.
__device__ __forceinline__ void jpeg_put(unsigned int* buf, unsigned int pos, unsigned int value, int len) {
    const unsigned long long v = (unsigned long long)value << (64 - len - (int)(pos & 31u));
    const unsigned int hi = (unsigned int)(v >> 32), lo = (unsigned int)v;
    atomicOr(&buf[pos >> 5], hi);
    if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}

// size category and the appended bits of a nonzero value (T.81 F.1.2.1): negative values are coded as value - 1, low bits
__device__ __forceinline__ int jpeg_category(int v, unsigned int* extra) {
    const int size = 32 - __clz(v < 0 ? -v : v);
    *extra = (unsigned int)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    return size;
}

// One block: DC difference, then a (run, size) symbol per nonzero AC coefficient found from the mask, ZRL for every 16 zeros in
// a run, EOB unless position 63 is nonzero.  EMIT = false only counts.  Returns the bits.
template <bool EMIT>
__device__ __forceinline__ unsigned int jpeg_code_block(const short* __restrict__ blk, unsigned long long mask, int pred,
                                                        const unsigned int* dc_table, const unsigned int* ac_table,
                                                        unsigned int* buf, unsigned int pos) {
    unsigned int bits = 0;
    {
        int diff = (int)blk[0] - pred;
        diff = max(-2047, min(2047, diff));
        unsigned int extra = 0;
        const int size = diff ? jpeg_category(diff, &extra) : 0;
        const unsigned int e = dc_table[size];
        const int len = (int)(e >> 16) + size;
        if (EMIT) jpeg_put(buf, pos, ((e & 0xffffu) << size) | extra, len);
        bits += len;
    }
    mask &= ~1ull;
    int prev = 0;
    while (mask) {
        const int p = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        int run = p - prev - 1;
        prev = p;
        const unsigned int zrl = ac_table[0xf0];
        while (run >= 16) {
            if (EMIT) jpeg_put(buf, pos + bits, zrl & 0xffffu, (int)(zrl >> 16));
            bits += zrl >> 16;
            run -= 16;
        }
        unsigned int extra;
        const int size = jpeg_category((int)blk[p], &extra);
        const unsigned int e = ac_table[(run << 4) | size];
        const int len = (int)(e >> 16) + size;
        if (EMIT) jpeg_put(buf, pos + bits, ((e & 0xffffu) << size) | extra, len);
        bits += len;
    }
    if (prev != 63) {
        const unsigned int eob = ac_table[0];
        if (EMIT) jpeg_put(buf, pos + bits, eob & 0xffffu, (int)(eob >> 16));
        bits += eob >> 16;
    }
    return bits;
}

// exclusive prefix sum over the 256 lanes of a workgroup, and the total; `part` is [5] words of LDS.  Every lane calls it.
__device__ __forceinline__ unsigned int jpeg_scan256(unsigned int v, unsigned int* part, unsigned int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();                                                         // (the previous call's readers are done)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    unsigned int before = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) before += w < wave ? part[w] : 0u;
    *total = part[0] + part[1] + part[2] + part[3];
    return before + inc - v;
}

__device__ __forceinline__ unsigned int jpeg_byte(const unsigned int* buf, unsigned int i) {
    return (buf[i >> 2] >> (24 - 8 * (i & 3u))) & 0xffu;
}

// grid N * MR, 256 lanes: interval = one MCU row of one frame; its bytes -> stage + interval * slot, its byte count -> lens
__global__ __launch_bounds__(256) void jpeg_interval_kernel(const short* __restrict__ coef, unsigned char* __restrict__ stage,
                                                            int* __restrict__ lens, long long slot, int MR, int MC) {
    __shared__ unsigned int buf[JPEG_BUF_WORDS];
    __shared__ unsigned int dc_table[2][12];
    __shared__ unsigned int ac_table[2][256];
    __shared__ unsigned int part[4];
    const int tid = threadIdx.x;
    const long long interval = blockIdx.x;
    const int restart = (int)(interval % MR);
    for (int i = tid; i < 24; i += 256) dc_table[i / 12][i % 12] = jpeg_huff.dc[i / 12][i % 12];
    for (int i = tid; i < 512; i += 256) ac_table[i >> 8][i & 255] = jpeg_huff.ac[i >> 8][i & 255];
    const short* row = coef + interval * MC * 384;
    unsigned char* out = stage + interval * slot;
    const int blocks = 6 * MC;
    unsigned int carry_bits = 0, carry_value = 0;                            // up to 7 bits not yet a byte (same in every lane)
    unsigned int written = 0;                                                // bytes of this interval in `out` so far
    for (int first = 0; first < blocks; first += JPEG_CHUNK) {
        const int b = first + tid;
        const bool active = b < blocks;
        const bool last = first + JPEG_CHUNK >= blocks;
        const int mcu = b / 6, k = b - 6 * mcu, comp = k >= 4;
        const short* blk = row + (long long)b * 64;
        unsigned long long mask = 0;
        int pred = 0;
        if (active) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const uint4 v = reinterpret_cast<const uint4*>(blk)[g];
                const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (w[e] & 0xffffu) mask |= 1ull << (8 * g + 2 * e);
                    if (w[e] >> 16) mask |= 1ull << (8 * g + 2 * e + 1);
                }
            }
            // the block before this one of the same component within the interval (prediction is 0 at its start)
            if (k >= 1 && k <= 3) pred = blk[-64];
            else if (mcu > 0) pred = k == 0 ? blk[-3 * 64] : blk[-6 * 64];
        }
        __syncthreads();                                                     // the tables; the previous chunk's readers of buf
        unsigned int bits = active ? jpeg_code_block<false>(blk, mask, pred, dc_table[comp], ac_table[comp], nullptr, 0) : 0u;
        unsigned int total;
        const unsigned int at = carry_bits + jpeg_scan256(bits, part, &total);
        const unsigned int end = carry_bits + total;                         // bits in buf after this chunk
        const unsigned int pad = last ? (8u - (end & 7u)) & 7u : 0u;
        const int words = (int)((end + pad + 31u) >> 5) + 1;
        const unsigned int head = carry_bits ? carry_value << (32 - carry_bits) : 0u;
        for (int i = tid; i < words; i += 256) buf[i] = i == 0 ? head : 0u;
        __syncthreads();
        if (active) jpeg_code_block<true>(blk, mask, pred, dc_table[comp], ac_table[comp], buf, at);
        if (tid == 0 && pad) jpeg_put(buf, end, (1u << pad) - 1u, (int)pad);  // 1-bits up to the byte boundary
        __syncthreads();
        // whole bytes leave, FF followed by 00: a lane takes `span` consecutive bytes
        const unsigned int nbytes = (end + pad) >> 3;
        const unsigned int span = (nbytes + 255u) / 256u;
        const unsigned int lo = min((unsigned int)tid * span, nbytes), hi = min(lo + span, nbytes);
        unsigned int ff = 0;
        for (unsigned int i = lo; i < hi; ++i) ff += jpeg_byte(buf, i) == 0xffu;
        unsigned int ff_total;
        unsigned int dst = written + lo + jpeg_scan256(ff, part, &ff_total);
        for (unsigned int i = lo; i < hi; ++i) {
            const unsigned int v = jpeg_byte(buf, i);
            out[dst++] = (unsigned char)v;
            if (v == 0xffu) out[dst++] = 0;
        }
        written += nbytes + ff_total;
        carry_bits = last ? 0u : end & 7u;
        carry_value = carry_bits ? jpeg_byte(buf, nbytes) >> (8 - carry_bits) : 0u;
    }
    if (tid == 0) {
        if (restart != MR - 1) {                                             // RSTm behind every interval but a frame's last
            out[written] = 0xff;
            out[written + 1] = (unsigned char)(0xd0 + (restart & 7));
            written += 2;
        }
        lens[interval] = (int)written;
    }
}

// one workgroup: starts[i] = sum of lens[0 .. i), offsets[n] = starts[n * MR], offsets[N] = the total
__global__ __launch_bounds__(256) void jpeg_offsets_kernel(const int* __restrict__ lens, long long* __restrict__ starts,
                                                           long long* __restrict__ offsets, long long intervals, int MR) {
    __shared__ unsigned int part[4];
    long long running = 0;
    for (long long first = 0; first < intervals; first += 256) {
        const long long i = first + threadIdx.x;
        const unsigned int v = i < intervals ? (unsigned int)lens[i] : 0u;
        unsigned int total;
        const unsigned int before = jpeg_scan256(v, part, &total);          // (256 intervals stay far below 2^32 bytes)
        if (i < intervals) {
            starts[i] = running + before;
            if (i % MR == 0) offsets[i / MR] = running + before;
        }
        running += total;
    }
    if (threadIdx.x == 0) offsets[intervals / MR] = running;
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const unsigned char* __restrict__ stage, const int* __restrict__ lens,
                                                        const long long* __restrict__ starts, unsigned char* __restrict__ scan,
                                                        long long slot) {
    const long long interval = blockIdx.x;
    const unsigned char* src = stage + interval * slot;
    unsigned char* dst = scan + starts[interval];
    const int len = lens[interval];
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
}

struct JpegPlan {
    int MR, MC;
    long long intervals, slot, coef_bytes, lens_bytes, starts_bytes, total;
    bool ok;
};

// slot: what one interval can come to -- every block at JPEG_BLOCK_BYTES, every byte an FF, the marker -- rounded up to 16
JpegPlan jpeg_plan(int N, int H, int W) {
    JpegPlan p = {};
    if (N <= 0 || H <= 0 || W <= 0) return p;
    p.MR = (H + 15) / 16;
    p.MC = (W + 15) / 16;
    p.intervals = (long long)N * p.MR;
    p.slot = (2ll * JPEG_BLOCK_BYTES * 6 * p.MC + 2 + 15) & ~15ll;
    if ((double)p.intervals * (double)p.slot > 4.0e18 || (double)p.intervals * p.MC * 768.0 > 4.0e18) return p;
    p.coef_bytes = p.intervals * p.MC * 768;                                 // [N, MR, MC, 6, 64] shorts
    p.lens_bytes = (p.intervals * 4 + 15) & ~15ll;
    p.starts_bytes = (p.intervals * 8 + 15) & ~15ll;
    p.total = p.coef_bytes + p.lens_bytes + p.starts_bytes + p.intervals * p.slot;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" long long msg_jpeg_workspace(int N, int H, int W) {
    const JpegPlan p = jpeg_plan(N, H, W);
    return p.ok ? p.total : -1;
}

extern "C" int msg_jpeg_scan_capacity(int N, int H, int W, long long* bytes) {
    const JpegPlan p = jpeg_plan(N, H, W);
    if (!bytes || !p.ok) return MSG_EINVAL;
    *bytes = p.intervals * p.slot;
    return MSG_OK;
}

extern "C" int msg_jpeg_encode(const unsigned char* rgb, const unsigned short* qtables, short* coef, unsigned char* scan,
                               long long* offsets, int N, int H, int W, void* ws, void* stream) {
    if (!rgb || !qtables || !scan || !offsets || !ws || N <= 0 || H <= 0 || W <= 0) return MSG_EINVAL;
    if ((((uintptr_t)ws) & 15u) || (((uintptr_t)coef) & 1u) || (((uintptr_t)offsets) & 7u)) return MSG_EINVAL;
    JpegQuant quant;
    for (int i = 0; i < 128; ++i) {
        if (qtables[i] < 1 || qtables[i] > 255) return MSG_EINVAL;
        quant.q[i] = qtables[i];
    }
    const JpegPlan p = jpeg_plan(N, H, W);
    if (!p.ok || p.intervals > 0x7fffffffll || N > 65535 || p.MR > 65535) return MSG_EINVAL;   // (the grids below)
    if (W > MSG_JPEG_MAX_WIDTH) return MSG_EUNSUPPORTED;
    unsigned char* base = (unsigned char*)ws;
    short* coef_ws = (short*)base;
    int* lens = (int*)(base + p.coef_bytes);
    long long* starts = (long long*)(base + p.coef_bytes + p.lens_bytes);
    unsigned char* stage = base + p.coef_bytes + p.lens_bytes + p.starts_bytes;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((p.MC + JPEG_GROUP - 1) / JPEG_GROUP), (unsigned)p.MR, (unsigned)N),
                       dim3(192), 0, s, rgb, quant, coef_ws, coef, H, W, p.MR, p.MC);
    hipLaunchKernelGGL(jpeg_interval_kernel, dim3((unsigned)p.intervals), dim3(256), 0, s, (const short*)coef_ws, stage, lens,
                       p.slot, p.MR, p.MC);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(256), 0, s, (const int*)lens, starts, offsets, p.intervals, p.MR);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)p.intervals), dim3(256), 0, s, (const unsigned char*)stage,
                       (const int*)lens, (const long long*)starts, scan, p.slot);
    return MSG_CHECK_LAUNCH();
}
