// Geometry and launchers of the device DEFLATE encoder (deflate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define DF_LANES 64                       // one wave per chunk
#define DF_SEG 516                        // bytes a lane parses: 2 * 258, and 129 words, an odd LDS stride
#define DF_CHUNK (DF_LANES * DF_SEG)      // 33024 input bytes per fragment (one stored block holds up to 65535)
#define DF_SLOT (DF_CHUNK + 16)           // workspace bytes per fragment: a fragment is never longer than its stored form, DF_CHUNK + 5
#define DF_SYMS 316                       // 286 literal/length + 30 distance table entries
#define DF_MAX_PITCH 32768
#define DF_MAX_HEADER_BITS 4096

struct DfPowers { uint32_t v[32]; };      // x^(2^k) mod the CRC-32 polynomial, for CRC concatenation

size_t rs_deflate_bound(size_t n);
size_t rs_deflate_workspace_bytes(int planes, size_t n);
int rs_launch_deflate_planes(const uint8_t* src, long plane_stride, long n, int planes, int pitch, const uint32_t* table, const uint32_t* header,
                             int header_bits, uint8_t* out, unsigned long long* offsets, unsigned long long* sizes, uint32_t* crcs, void* workspace,
                             hipStream_t st);
