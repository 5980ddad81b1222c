// DEFLATE (RFC 1951) encoder for byte planes that are almost all runs and repeated rows (uint8 masks, bit-packed masks): the compressed member of a
// .npz / .gz is produced on the device and only its bytes cross the bus (inference/npz_writer.py writes the container around it).
//
//   deflate_encode_kernel    one block (one wave) per chunk of DF_CHUNK input bytes of one plane -> one byte-aligned fragment in the workspace, its size and
//                            the CRC-32 of the chunk
//   deflate_scan_kernel      one block: per plane the stream size, the CRC-32 of the plane and the place of every fragment; then the plane offsets
//   deflate_compact_kernel   fragments -> one contiguous buffer; the closing block of every stream
//
// Stream of a plane of n bytes: the fragments of its ceil(n / DF_CHUNK) chunks, then `01 00 00 FF FF` (an empty stored block with BFINAL = 1).
// Fragment of a chunk of m bytes, whichever is shorter (the first on a tie):
//   coded   one Huffman block: the caller's header bits (BFINAL = 0, BTYPE, for BTYPE 10 the code lengths), the tokens, the end-of-block code; then an
//           empty stored block that brings the stream back to a byte boundary: three zero bits, zero bits up to the byte, 00 00 FF FF
//   stored  00, m as two bytes, ~m as two bytes, the m bytes
// Tokens: lane l of the block parses segment l of the chunk, DF_SEG bytes, on its own and from left to right.  At plane position i with r bytes left in the
// segment, L1 = the number of k < min(r, 258) leading positions with x[i + k] == x[i + k - 1] (0 when i = 0) and Lp the same with distance `pitch` (0 when
// pitch < 2 or i < pitch).  L = max(L1, Lp); L >= 3 emits a match of length L at distance 1 if L1 >= Lp, else at distance pitch, and moves on by L; otherwise
// the literal x[i], and moves on by 1.  A match refers to input positions, so it may reach into the chunk before (never before the plane).
// The code table is an argument: 286 literal/length and 30 distance entries, (bits << 24) | code with the code bit-reversed (DEFLATE packs Huffman codes
// from their most significant bit; everything else, and this encoder's bit buffer, is least-significant-bit first).
// Two passes over the segment: the first counts the bits, a wave prefix sum places every lane's first bit, the second writes them with LDS atomic OR into
// zeroed words.  DF_SEG = 516 = 2 * 258 bytes = 129 words: 64 lanes that walk their segments in step touch 64 different banks.
// Integer arithmetic only: the same input gives the same bytes.
#include "common.hpp"
#include "deflate.hpp"

#define DF_POLY 0xEDB88320u

// a(x) * b(x) mod the CRC-32 polynomial, reflected bit order (bit 31 = x^0)
__host__ __device__ static inline uint32_t df_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ DF_POLY : b >> 1;
    }
    return p;
}
// x^(8 * nbytes) mod the polynomial; pw.v[k] = x^(2^k)
__host__ __device__ static inline uint32_t df_xpow8(const DfPowers& pw, unsigned long long nbytes) {
    uint32_t p = 0x80000000u;
    for (int k = 3; nbytes; nbytes >>= 1, ++k)
        if (nbytes & 1ull) p = df_mulmod(pw.v[k & 31], p);
    return p;
}
// crc32(A || B) from crc32(A), crc32(B) and len(B)
__host__ __device__ static inline uint32_t df_crc_shift(const DfPowers& pw, uint32_t crc_a, unsigned long long len_b) {
    return df_mulmod(df_xpow8(pw, len_b), crc_a);
}

DfPowers df_powers() {
    DfPowers pw;
    uint32_t p = 0x40000000u;                                    // x^1
    for (int k = 0; k < 32; ++k) { pw.v[k] = p; p = df_mulmod(p, p); }
    return pw;
}

__device__ __forceinline__ unsigned long long df_wave_incl_scan(unsigned long long v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t df_wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

// (symbol, extra bits, extra value) of a match length 3..258 and of a distance 1..32768 (RFC 1951 section 3.2.5)
__device__ __forceinline__ void df_len_sym(int len, int& sym, int& eb, int& ev) {
    const int l = len - 3;
    if (len == 258) { sym = 285; eb = 0; ev = 0; }
    else if (l < 4) { sym = 257 + l; eb = 0; ev = 0; }
    else { eb = (31 - __clz(l)) - 2; sym = 261 + 4 * eb + ((l >> eb) & 3); ev = l & ((1 << eb) - 1); }
}
__device__ __forceinline__ void df_dist_sym(int dist, int& sym, int& eb, int& ev) {
    const int d = dist - 1;
    if (d < 4) { sym = d; eb = 0; ev = 0; }
    else { eb = (31 - __clz(d)) - 1; sym = 2 * (eb + 1) + ((d >> eb) & 1); ev = d & ((1 << eb) - 1); }
}

// LSB-first bit writer of one lane: whole and partial words are OR-ed into zeroed LDS words, so neighbours may share a word
struct DfBits {
    uint32_t* out;
    unsigned long long acc;
    int nacc;
    unsigned w;
    __device__ __forceinline__ void start(uint32_t* o, unsigned long long bitpos) { out = o; w = (unsigned)(bitpos >> 5); nacc = (int)(bitpos & 31); acc = 0; }
    __device__ __forceinline__ void put(uint32_t v, int nb) {      // nb <= 32, v < 2^nb
        acc |= (unsigned long long)v << nacc;
        nacc += nb;
        if (nacc >= 32) { atomicOr(&out[w], (uint32_t)acc); ++w; acc >>= 32; nacc -= 32; }
    }
    __device__ __forceinline__ void flush() { if (nacc > 0 && (uint32_t)acc) atomicOr(&out[w], (uint32_t)acc); }
    __device__ __forceinline__ unsigned long long pos() const { return ((unsigned long long)w << 5) + (unsigned)nacc; }
};

// One pass over the segment [q0, q1) of the staged bytes `in` (in[q] = plane byte i0 + q): the bits of its tokens; WRITE emits them too.
template <bool WRITE>
__device__ __forceinline__ unsigned df_parse(const uint8_t* in, int q0, int q1, long i0, int pitch, const uint32_t* tab, uint32_t dcode1, int dbits1,
                                             uint32_t dcodep, int dbitsp, DfBits& bw) {
    unsigned bits = 0;
    int q = q0;
    while (q < q1) {
        const int lim = min(q1 - q, 258);
        const uint8_t b = in[q];
        int l1 = 0, lp = 0;
        if (i0 + q >= 1) { while (l1 < lim && in[q + l1] == in[q + l1 - 1]) ++l1; }
        if (pitch >= 2 && i0 + q >= pitch) { while (lp < lim && in[q + lp] == in[q + lp - pitch]) ++lp; }
        const int L = max(l1, lp);
        if (L >= 3) {
            int sym, eb, ev;
            df_len_sym(L, sym, eb, ev);
            const uint32_t t = tab[sym];
            const bool one = l1 >= lp;
            bits += (t >> 24) + eb + (one ? dbits1 : dbitsp);
            if (WRITE) {
                bw.put((t & 0xFFFFFFu) | ((uint32_t)ev << (t >> 24)), (int)(t >> 24) + eb);
                bw.put(one ? dcode1 : dcodep, one ? dbits1 : dbitsp);
            }
            q += L;
        } else {
            const uint32_t t = tab[b];
            bits += t >> 24;
            if (WRITE) bw.put(t & 0xFFFFFFu, (int)(t >> 24));
            q += 1;
        }
    }
    return bits;
}

// LDS: [staged input: back + DF_CHUNK bytes, rounded up to words][output words: DF_SLOT bytes][code table 316 words][CRC table 256 words]
__global__ __launch_bounds__(DF_LANES) void deflate_encode_kernel(const uint8_t* __restrict__ src, long plane_stride, long n, int pitch, int nchunks,
                                                                  const uint32_t* __restrict__ table, const uint32_t* __restrict__ header, int header_bits,
                                                                  uint8_t* __restrict__ slots, uint32_t* __restrict__ frag_size, uint32_t* __restrict__ frag_crc,
                                                                  int in_words, DfPowers pw) {
    extern __shared__ uint32_t df_lds[];
    uint32_t* in_w = df_lds;
    uint32_t* out_w = df_lds + in_words;
    uint32_t* tab = out_w + DF_SLOT / 4;
    uint32_t* crc_tab = tab + DF_SYMS;
    const uint8_t* in = (const uint8_t*)in_w;
    const int lane = threadIdx.x;
    const int chunk = blockIdx.x, plane = blockIdx.y;
    const long cs = (long)chunk * DF_CHUNK;
    const int m = (int)min((long)DF_CHUNK, n - cs);
    const int back = (int)min((long)max(pitch, 1), cs);           // bytes in front of the chunk that a match may look at
    const int total = back + m;
    const long i0 = cs - back;                                    // plane position of in[0]
    const uint8_t* g = src + (size_t)plane * (size_t)plane_stride + i0;

    // stage: aligned global words, shifted into place; the last total % 4 bytes one by one.  No byte outside [g, g + total) is in a word that is read
    // unless that word also holds a byte inside.
    {
        const unsigned sh = (unsigned)((uintptr_t)g & 3);
        const uint32_t* ga = (const uint32_t*)(g - sh);
        const int full = total >> 2;
        if (sh == 0) {
            for (int k = lane; k < full; k += DF_LANES) in_w[k] = ga[k];
        } else {
            for (int k = lane; k < full; k += DF_LANES) {
                const uint32_t lo = ga[k], hi = ga[k + 1];
                in_w[k] = (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
            }
        }
        if (lane == 0 && (total & 3)) {
            uint32_t v = 0;
            for (int j = 0; j < (total & 3); ++j) v |= (uint32_t)g[full * 4 + j] << (8 * j);
            in_w[full] = v;
        }
    }
    for (int k = lane; k < DF_SYMS; k += DF_LANES) tab[k] = table[k];
    for (int k = lane; k < 256; k += DF_LANES) {
        uint32_t c = (uint32_t)k;
#pragma unroll
        for (int j = 0; j < 8; ++j) c = (c & 1u) ? (c >> 1) ^ DF_POLY : c >> 1;
        crc_tab[k] = c;
    }
    __syncthreads();

    const int q0 = min(back + lane * DF_SEG, total), q1 = min(q0 + DF_SEG, total);
    // CRC-32 of the chunk: every lane's segment on its own, shifted by the bytes that follow it in the chunk, XOR over the lanes
    uint32_t crc = 0;
    if (q1 > q0) {
        uint32_t c = 0xFFFFFFFFu;
        for (int q = q0; q < q1; ++q) c = crc_tab[(c ^ in[q]) & 0xFFu] ^ (c >> 8);
        crc = df_crc_shift(pw, ~c, (unsigned long long)(total - q1));
    }
    crc = df_wave_xor(crc);

    int dsym, deb, dev;
    df_dist_sym(1, dsym, deb, dev);
    const uint32_t t1 = tab[286 + dsym];
    const uint32_t dcode1 = t1 & 0xFFFFFFu;
    const int dbits1 = (int)(t1 >> 24);
    df_dist_sym(pitch >= 2 ? pitch : 1, dsym, deb, dev);
    const uint32_t tp = tab[286 + dsym];
    const uint32_t dcodep = (tp & 0xFFFFFFu) | ((uint32_t)dev << (tp >> 24));
    const int dbitsp = (int)(tp >> 24) + deb;

    DfBits bw;
    const unsigned mine = df_parse<false>(in, q0, q1, i0, pitch, tab, dcode1, dbits1, dcodep, dbitsp, bw);
    const unsigned long long incl = df_wave_incl_scan(mine, lane);
    const unsigned long long all = __shfl(incl, DF_LANES - 1, 64);
    const uint32_t eob = tab[256];
    const unsigned long long block_bits = (unsigned long long)header_bits + all + (eob >> 24);
    const unsigned coded_bytes = (unsigned)((block_bits + 3 + 7) >> 3) + 4;
    const unsigned stored_bytes = (unsigned)m + 5;
    uint8_t* slot = slots + ((size_t)plane * nchunks + chunk) * DF_SLOT;
    const bool coded = coded_bytes <= stored_bytes;                // wave-uniform
    if (coded) {
        const int words = (int)((coded_bytes + 3) >> 2);
        for (int k = lane; k < words; k += DF_LANES) out_w[k] = 0;
        __syncthreads();
        bw.start(out_w, lane == 0 ? 0ull : (unsigned long long)header_bits + incl - mine);
        if (lane == 0) {
            for (int h = 0; h < header_bits; h += 32) {
                const int nb = min(32, header_bits - h);
                const uint32_t v = header[h >> 5];
                bw.put(nb == 32 ? v : (v & ((1u << nb) - 1u)), nb);
            }
        }
        df_parse<true>(in, q0, q1, i0, pitch, tab, dcode1, dbits1, dcodep, dbitsp, bw);
        if (lane == DF_LANES - 1) bw.put(eob & 0xFFFFFFu, (int)(eob >> 24));
        bw.flush();
        if (lane == DF_LANES - 1) {                                // 00 00 FF FF at the byte after the three header bits of the empty stored block
            const unsigned at = coded_bytes - 2;
            atomicOr(&out_w[at >> 2], 0xFFu << (8 * (at & 3)));
            atomicOr(&out_w[(at + 1) >> 2], 0xFFu << (8 * ((at + 1) & 3)));
        }
        __syncthreads();
        uint32_t* sw = (uint32_t*)slot;
        for (int k = lane; k < words; k += DF_LANES) sw[k] = out_w[k];
    } else {
        if (lane == 0) {
            slot[0] = 0; slot[1] = (uint8_t)(m & 0xFF); slot[2] = (uint8_t)(m >> 8);
            slot[3] = (uint8_t)(~m & 0xFF); slot[4] = (uint8_t)((~m >> 8) & 0xFF);
        }
        for (int j = lane; j < m; j += DF_LANES) slot[5 + j] = in[back + j];
    }
    if (lane == 0) {
        frag_size[(size_t)plane * nchunks + chunk] = coded ? coded_bytes : stored_bytes;
        frag_crc[(size_t)plane * nchunks + chunk] = crc;
    }
}

// Per plane (one wave each, four at a time): size of the stream, CRC-32 of the plane, start of every fragment inside the stream.  Then the start of every
// stream inside `out` (the streams lie back to back in plane order).
__global__ __launch_bounds__(256) void deflate_scan_kernel(const uint32_t* __restrict__ frag_size, const uint32_t* __restrict__ frag_crc,
                                                           unsigned long long* __restrict__ frag_off, int planes, int nchunks, long n,
                                                           unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ sizes,
                                                           uint32_t* __restrict__ crcs, DfPowers pw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < planes; p += 4) {
        unsigned long long carry = 0;
        uint32_t crc = 0;
        for (int c0 = 0; c0 < nchunks; c0 += 64) {
            const int c = c0 + lane;
            const unsigned long long sz = c < nchunks ? frag_size[(size_t)p * nchunks + c] : 0;
            const unsigned long long incl = df_wave_incl_scan(sz, lane);
            if (c < nchunks) {
                frag_off[(size_t)p * nchunks + c] = carry + incl - sz;
                const long end = min((long)(c + 1) * DF_CHUNK, n);
                crc ^= df_crc_shift(pw, frag_crc[(size_t)p * nchunks + c], (unsigned long long)(n - end));
            }
            carry += __shfl(incl, 63, 64);
        }
        crc = df_wave_xor(crc);
        if (lane == 0) { sizes[p] = carry + 5; crcs[p] = crc; }
    }
    __syncthreads();
    if (wave == 0) {
        unsigned long long carry = 0;
        for (int p0 = 0; p0 < planes; p0 += 64) {
            const int p = p0 + lane;
            const unsigned long long sz = p < planes ? sizes[p] : 0;
            const unsigned long long incl = df_wave_incl_scan(sz, lane);
            if (p < planes) offsets[p] = carry + incl - sz;
            carry += __shfl(incl, 63, 64);
        }
    }
}

// Block (c, p) copies fragment c of plane p to its place; the block of the last fragment (block 0 of an empty plane) appends the closing block.
__global__ __launch_bounds__(256) void deflate_compact_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ frag_size,
                                                              const unsigned long long* __restrict__ frag_off, int nchunks,
                                                              const unsigned long long* __restrict__ offsets, const unsigned long long* __restrict__ sizes,
                                                              uint8_t* __restrict__ out) {
    const int c = blockIdx.x, p = blockIdx.y;
    uint8_t* dst_plane = out + offsets[p];
    if (c < nchunks) {
        const size_t f = (size_t)p * nchunks + c;
        const uint8_t* s = slots + f * DF_SLOT;
        uint8_t* d = dst_plane + frag_off[f];
        const unsigned sz = frag_size[f];
        const unsigned head = min(sz, (unsigned)((4 - ((uintptr_t)d & 3)) & 3));     // bytes up to the first aligned word of the destination
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        const unsigned words = (sz - head) >> 2;
        uint32_t* dw = (uint32_t*)(d + head);
        for (unsigned k = threadIdx.x; k < words; k += 256) {
            const uint8_t* sb = s + head + 4 * k;
            dw[k] = (uint32_t)sb[0] | ((uint32_t)sb[1] << 8) | ((uint32_t)sb[2] << 16) | ((uint32_t)sb[3] << 24);
        }
        const unsigned done = head + 4 * words;
        if (threadIdx.x < sz - done) d[done + threadIdx.x] = s[done + threadIdx.x];
    }
    if (c == max(nchunks, 1) - 1 && threadIdx.x < 5) {
        const uint8_t closing[5] = {1, 0, 0, 0xFF, 0xFF};
        dst_plane[sizes[p] - 5 + threadIdx.x] = closing[threadIdx.x];
    }
}

static inline int df_chunks(long n) { return (int)((n + DF_CHUNK - 1) / DF_CHUNK); }

size_t rs_deflate_bound(size_t n) { return n + 5 * ((n + DF_CHUNK - 1) / DF_CHUNK) + 5; }

// workspace: [fragment slots][fragment sizes u32][fragment CRCs u32][fragment offsets u64], each part 16-byte aligned
static inline size_t df_align16(size_t v) { return (v + 15) & ~(size_t)15; }
size_t rs_deflate_workspace_bytes(int planes, size_t n) {
    const size_t f = (size_t)planes * ((n + DF_CHUNK - 1) / DF_CHUNK);
    return f * DF_SLOT + 2 * df_align16(f * 4) + df_align16(f * 8) + 16;
}

int rs_launch_deflate_planes(const uint8_t* src, long plane_stride, long n, int planes, int pitch, const uint32_t* table, const uint32_t* header,
                             int header_bits, uint8_t* out, unsigned long long* offsets, unsigned long long* sizes, uint32_t* crcs, void* workspace,
                             hipStream_t st) {
    static const DfPowers pw = df_powers();
    const int nchunks = df_chunks(n);
    const size_t f = (size_t)planes * nchunks;
    uint8_t* slots = (uint8_t*)workspace;
    uint32_t* frag_size = (uint32_t*)(slots + f * DF_SLOT);
    uint32_t* frag_crc = (uint32_t*)((uint8_t*)frag_size + df_align16(f * 4));
    unsigned long long* frag_off = (unsigned long long*)((uint8_t*)frag_crc + df_align16(f * 4));
    if (nchunks > 0) {
        const int in_words = (DF_CHUNK + (pitch > 1 ? pitch : 1) + 3) / 4 + 1;
        const size_t smem = ((size_t)in_words + DF_SLOT / 4 + DF_SYMS + 256) * 4;
        if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)deflate_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(deflate_encode_kernel, dim3((unsigned)nchunks, (unsigned)planes), dim3(DF_LANES), smem, st, src, plane_stride, n, pitch, nchunks,
                           table, header, header_bits, slots, frag_size, frag_crc, in_words, pw);
    }
    hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(256), 0, st, frag_size, frag_crc, frag_off, planes, nchunks, n, offsets, sizes, crcs, pw);
    hipLaunchKernelGGL(deflate_compact_kernel, dim3((unsigned)(nchunks > 0 ? nchunks : 1), (unsigned)planes), dim3(256), 0, st, slots, frag_size, frag_off,
                       nchunks, offsets, sizes, out);
    return rs_check_launch();
}
