// lm_png.hip -- 8-bit grayscale PNG encode / decode on the device: the frame hand-off between the pipeline's step scripts
// (FCN_lecturenet_binarizer.py:56 writes compressed_frames, helper.py:31 reads them, cc_stability_estimator.py:678 writes
// the reconstructed frames; paths relative to ACCESS2021_release).  Host zlib does the same job in
// lecturemath_amd/png.py and stays the default.
//
// Encoder (lm_png_encode): every row is "Up"-filtered (type 2) and tokenised on its own as literals plus distance-1 matches
// (runs of one byte value, greedy, 258 at most), all in ONE fixed-Huffman deflate block.  Rows never reference each other,
// so the work is a thread per row, twice:
//   lm_k_png_rows<0>   bit count of every row + the row's adler32 terms (sum of bytes, sum of index * byte)
//   lm_k_png_frame     per frame (block): exclusive scan of the row bit counts, adler32 of the frame from the row terms,
//                      the file size; zeroes the deflate bytes and writes signature, IHDR (+ CRC), IDAT header, zlib header,
//                      block header, adler32 and IEND
//   lm_k_png_rows<1>   every row writes its tokens at its bit offset (words shared with a neighbour row by atomicOr)
//   lm_k_png_crc       per frame (block): CRC-32 of the IDAT chunk as per-thread segment CRCs combined with zlib's
//                      crc32_combine arithmetic (multiplication by x^(8 * bytes after the segment) modulo the polynomial)
// A literal costs 8 or 9 bits and a match at least 3 bytes for at most 18 bits, so a row of W + 1 bytes never takes more than
// 9 * (W + 1) bits: lm_png_encode_bound is 63 bytes of framing + ceil((10 + 9 * H * (W + 1)) / 8), rounded up to 16.
//
// Decoder (lm_png_decode): any 8-bit gray, non-interlaced PNG.
//   lm_k_png_gather    a wave per file walks the chunks inside [offset, offset + length), checks the signature and IHDR and
//                      concatenates the IDAT payloads into a per-frame scratch slot (a stream longer than the slot is
//                      reported UNSUPPORTED, and the caller decodes that file on the host)
//   lm_k_png_inflate   a wave per file runs inflate (stored, fixed and dynamic blocks; canonical-code decoding as in zlib's
//                      puff.c).  Every lane decodes the same symbols (wave-uniform control flow); the output goes through a
//                      32 KiB LDS ring (the deflate window), literals written by lane 0, matches copied by all lanes, and
//                      full 8 KiB ring chunks are flushed to the raw scratch
//   lm_k_png_unfilter  a block per frame, rows in order: None / Up rows by all threads, Sub / Average / Paeth rows serially
//                      from LDS; also checks the zlib adler32 of the raw stream
// Chunk CRCs are NOT checked by the decoder (the zlib adler32 is).  A frame's status is LM_PNG_OK, LM_PNG_UNSUPPORTED (other
// colour types, bit depths, interlace) or LM_PNG_CORRUPT (bad signature / chunk layout / zlib header / Huffman table,
// distance before the start of the output, truncated data, more or less data than the frame holds, wrong adler32, IHDR
// dimensions other than the expected ones).  Every read of a file is inside [offset, offset + length); every write is inside the
// frame's own slots.
#include "lm_common.h"

#ifndef LM_DYN_SMEM
#if LM_HIP_EMULATED
extern char* lm_emu_dynsmem;
#define LM_DYN_SMEM(name) char* name = lm_emu_dynsmem
#else
#define LM_DYN_SMEM(name) extern __shared__ __attribute__((aligned(16))) char name[]
#endif
#endif

#if LM_HIP_EMULATED
#define LM_PNG_TABLE static const
#else
#define LM_PNG_TABLE __constant__ static const
#endif

// LM_PNG_OK / LM_PNG_UNSUPPORTED / LM_PNG_CORRUPT: include/lecturemath_amd.h

#define LM_PNG_HEAD 43          // signature 8 + IHDR chunk 25 + IDAT length/tag 8 + zlib header 2: first deflate byte
#define LM_PNG_TAIL 20          // adler32 4 + IDAT CRC 4 + IEND chunk 12
#define LM_PNG_MAX_W 16384      // two rows in LDS for the unfilter kernel
#define LM_PNG_ADLER 65521u
#define LM_PNG_CRC_POLY 0xedb88320u

static inline long long lm_png_raw_bytes(int w, int h) { return (long long)h * (w + 1); }

// ---------------------------------------------------------------------------------------------------------------------
// shared arithmetic
// ---------------------------------------------------------------------------------------------------------------------

// a(x) * b(x) modulo the CRC-32 polynomial, reflected bit order (zlib's multmodp)
LM_DEV uint32_t lm_crc_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ LM_PNG_CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 * n) modulo the polynomial
LM_DEV uint32_t lm_crc_x8n(unsigned long long n)
{
    uint32_t p = 1u << 31;          // x^0
    uint32_t sq = 1u << 23;         // x^8
    while (n) {
        if (n & 1) p = lm_crc_multmodp(sq, p);
        n >>= 1;
        if (n) sq = lm_crc_multmodp(sq, sq);
    }
    return p;
}

LM_DEV uint32_t lm_crc_bitwise(uint32_t c, const uint8_t* p, int n)
{
    for (int i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (LM_PNG_CRC_POLY & (0u - (c & 1u)));
    }
    return c;
}

LM_DEV void lm_put_be32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------------------------------
// encoder
// ---------------------------------------------------------------------------------------------------------------------

// fixed-Huffman literal/length code of symbol s, bit-reversed for LSB-first packing; returns the length
LM_DEV int lm_fixed_code(int s, uint32_t* code)
{
    uint32_t c;
    int len;
    if (s < 144) { c = 0x30u + s; len = 8; }
    else if (s < 256) { c = 0x190u + (s - 144); len = 9; }
    else if (s < 280) { c = (uint32_t)(s - 256); len = 7; }
    else { c = 0xc0u + (s - 280); len = 8; }
    *code = __brev(c) >> (32 - len);
    return len;
}

// bits (value, count) of a distance-1 match of length L (3..258): length code + extra bits + the 5-bit distance code 0
LM_DEV int lm_match_bits(int L, unsigned long long* bits)
{
    int sym, ebits = 0, extra = 0;
    if (L == 258) sym = 285;
    else {
        const int l = L - 3;
        if (l < 8) sym = 257 + l;
        else {
            ebits = (31 - __clz(l)) - 2;
            const int top = (l >> ebits) & 3;
            sym = 257 + 4 * ebits + 4 + top;
            extra = l - ((4 + top) << ebits);
        }
    }
    uint32_t c;
    const int n = lm_fixed_code(sym, &c);
    *bits = (unsigned long long)c | ((unsigned long long)extra << n);   // distance code 0: five zero bits
    return n + ebits + 5;
}

// bit sink of the row tokeniser: counts (WRITE = 0) or packs into the frame's slot (WRITE = 1)
template <int WRITE>
struct LmBitSink {
    unsigned long long bits = 0;     // total bits (count mode)
    uint32_t* words = nullptr;       // slot as 32-bit words
    long long wp = 0;                // current word
    unsigned long long acc = 0;
    int fill = 0;
    bool first = true;

    __device__ __forceinline__ void put(unsigned long long v, int n)
    {
        if (!WRITE) { bits += n; return; }
        acc |= v << fill;
        fill += n;
        while (fill >= 32) {
            const uint32_t w = (uint32_t)acc;
            if (first) { if (w) atomicOr(words + wp, w); first = false; }   // may share the word with the row before
            else words[wp] = w;                                                // wholly this row's
            acc >>= 32;
            fill -= 32;
            wp++;
        }
    }
    __device__ __forceinline__ void finish()
    {
        if (WRITE && fill > 0 && (uint32_t)acc) atomicOr(words + wp, (uint32_t)acc);   // shared with the next row / the trailer
    }
};

template <int WRITE>
LM_DEV void lm_lit(LmBitSink<WRITE>& s, int v)
{
    uint32_t c;
    const int n = lm_fixed_code(v, &c);
    s.put(c, n);
}

template <int WRITE>
LM_DEV void lm_flush_run(LmBitSink<WRITE>& s, int prev, int run)
{
    while (run >= 3) {
        const int L = run < 258 ? run : 258;
        unsigned long long b;
        const int n = lm_match_bits(L, &b);
        s.put(b, n);
        run -= L;
    }
    for (; run > 0; run--) lm_lit(s, prev);
}

// one thread per (frame, row).  Count pass: rowbits = bits of the row's tokens, adl = (sum of the row's zlib bytes,
// sum of local index * byte), both mod 65521.  Write pass: the tokens at bit LM_PNG_HEAD * 8 + 3 + rowoff of the slot.
template <int WRITE>
__global__ void __launch_bounds__(256) lm_k_png_rows(const uint8_t* __restrict__ frames, int W, int H, int n, uint32_t* __restrict__ rowbits,
                                                     uint32_t* __restrict__ adl, const uint32_t* __restrict__ rowoff, uint8_t* __restrict__ out,
                                                     long long capacity)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long long)n * H) return;
    const int f = (int)(r / H), y = (int)(r - (long long)f * H);
    const uint8_t* cur = frames + r * W;
    const uint8_t* up = y > 0 ? cur - W : nullptr;
    LmBitSink<WRITE> s;
    if (WRITE) {
        const long long bit = (long long)LM_PNG_HEAD * 8 + 3 + rowoff[r];
        s.words = (uint32_t*)(out + (long long)f * capacity);
        s.wp = bit >> 5;
        s.fill = (int)(bit & 31);
    }
    // filter byte 2, then cur - up
    lm_lit(s, 2);
    int prev = 2, run = 0;
    unsigned long long s1 = 2, s2 = 0;
    for (int x = 0; x < W; x++) {
        const int d = (int)(uint8_t)(cur[x] - (up ? up[x] : 0));
        if (!WRITE) { s1 += d; s2 += (unsigned long long)(x + 1) * d; }
        if (d == prev) {
            if (++run == 258) { lm_flush_run(s, prev, run); run = 0; }
        } else {
            lm_flush_run(s, prev, run);
            lm_lit(s, d);
            prev = d;
            run = 0;
        }
    }
    lm_flush_run(s, prev, run);
    s.finish();
    if (!WRITE) {
        rowbits[r] = (uint32_t)s.bits;
        adl[2 * r] = (uint32_t)(s1 % LM_PNG_ADLER);
        adl[2 * r + 1] = (uint32_t)(s2 % LM_PNG_ADLER);
    }
}

#define LM_PNG_FT 256
// a block per frame: scan, adler32, sizes, framing bytes.  The deflate bytes are zeroed first (the write pass ORs into them).
__global__ void __launch_bounds__(LM_PNG_FT) lm_k_png_frame(int W, int H, const uint32_t* __restrict__ rowbits, const uint32_t* __restrict__ adl,
                                                            uint32_t* __restrict__ rowoff, uint8_t* __restrict__ out, long long capacity,
                                                            int64_t* __restrict__ sizes, uint32_t* __restrict__ dbytes)
{
    __shared__ unsigned long long s_bits[LM_PNG_FT];
    __shared__ unsigned long long s_a[LM_PNG_FT], s_b[LM_PNG_FT];
    const int f = blockIdx.x, t = threadIdx.x;
    const long long base = (long long)f * H;
    const int per = (H + LM_PNG_FT - 1) / LM_PNG_FT;
    const int y0 = t * per < H ? t * per : H, y1 = y0 + per < H ? y0 + per : H;
    const unsigned long long row_len = (unsigned long long)W + 1, total = row_len * H;
    unsigned long long bits = 0, a = 0, b = 0;
    for (int y = y0; y < y1; y++) {
        bits += rowbits[base + y];
        const unsigned long long S = adl[2 * (base + y)], T = adl[2 * (base + y) + 1];
        // the row's bytes sit at stream offsets y * (W + 1) + j: B += (total - offset) * byte, summed as (total - start) * S - T
        const unsigned long long rem = (total - (unsigned long long)y * row_len) % LM_PNG_ADLER;
        a += S;
        b += rem * S + (LM_PNG_ADLER - T);
    }
    s_bits[t] = bits;
    s_a[t] = a % LM_PNG_ADLER;
    s_b[t] = b % LM_PNG_ADLER;
    __syncthreads();
    // exclusive prefix of the thread totals (serial over 256 values in every thread: cheap next to the rows)
    unsigned long long off = 0;
    for (int i = 0; i < t; i++) off += s_bits[i];
    for (int y = y0; y < y1; y++) {
        rowoff[base + y] = (uint32_t)off;
        off += rowbits[base + y];
    }
    unsigned long long all = 0, A = 1, B = total % LM_PNG_ADLER;
    for (int i = 0; i < LM_PNG_FT; i++) { all += s_bits[i]; A += s_a[i]; B += s_b[i]; }
    A %= LM_PNG_ADLER;
    B %= LM_PNG_ADLER;
    const unsigned long long dbits = 3 + all + 7;     // block header, rows, end-of-block code (seven zero bits)
    const long long D = (long long)((dbits + 7) / 8);
    uint8_t* o = out + (long long)f * capacity;
    for (long long i = LM_PNG_HEAD + 1 + t; i < LM_PNG_HEAD + D; i += LM_PNG_FT) o[i] = 0;
    if (t == 0) {
        const long long size = LM_PNG_HEAD + D + LM_PNG_TAIL;
        sizes[f] = size;
        dbytes[f] = (uint32_t)D;
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
        for (int i = 0; i < 8; i++) o[i] = sig[i];
        uint8_t ihdr[17] = {'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0};
        lm_put_be32(ihdr + 4, (uint32_t)W);
        lm_put_be32(ihdr + 8, (uint32_t)H);
        lm_put_be32(o + 8, 13);
        for (int i = 0; i < 17; i++) o[12 + i] = ihdr[i];
        lm_put_be32(o + 29, lm_crc_bitwise(0xffffffffu, ihdr, 17) ^ 0xffffffffu);
        lm_put_be32(o + 33, (uint32_t)(2 + D + 4));
        o[37] = 'I'; o[38] = 'D'; o[39] = 'A'; o[40] = 'T';
        o[41] = 0x78; o[42] = 0x01;                    // zlib: deflate, 32 KiB window, no dictionary
        o[LM_PNG_HEAD] = 0x03;                         // BFINAL = 1, BTYPE = 01 (fixed Huffman)
        uint8_t* tail = o + LM_PNG_HEAD + D;
        lm_put_be32(tail, (uint32_t)((B << 16) | A));
        const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; i++) tail[8 + i] = iend[i];
    }
}

// a block per frame: CRC-32 of the IDAT chunk's tag + data (bytes 37 .. 43 + D + 4)
__global__ void __launch_bounds__(LM_PNG_FT) lm_k_png_crc(uint8_t* __restrict__ out, long long capacity, const uint32_t* __restrict__ dbytes)
{
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_part[LM_PNG_FT];
    const int f = blockIdx.x, t = threadIdx.x;
    {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (LM_PNG_CRC_POLY & (0u - (c & 1u)));
        s_tab[t] = c;
    }
    __syncthreads();
    uint8_t* o = out + (long long)f * capacity;
    const long long start = 37, len = 4 + 2 + (long long)dbytes[f] + 4;
    const long long per = (len + LM_PNG_FT - 1) / LM_PNG_FT;
    const long long s0 = t * per < len ? t * per : len, s1 = s0 + per < len ? s0 + per : len;
    uint32_t c = 0xffffffffu;
    for (long long i = s0; i < s1; i++) c = s_tab[(c ^ o[start + i]) & 0xff] ^ (c >> 8);
    c ^= 0xffffffffu;
    // crc(S_0 .. S_k) = XOR_k crc(S_k) * x^(8 * bytes after S_k); an empty segment contributes crc("") = 0
    s_part[t] = s1 > s0 ? lm_crc_multmodp(lm_crc_x8n((unsigned long long)(len - s1)), c) : 0u;
    __syncthreads();
    if (t == 0) {
        uint32_t x = 0;
        for (int i = 0; i < LM_PNG_FT; i++) x ^= s_part[i];
        lm_put_be32(o + start + len, x);
    }
}

// packs n files from their slots into one buffer at the given offsets (one block per file)
__global__ void __launch_bounds__(256) lm_k_png_pack(const uint8_t* __restrict__ slots, long long capacity, const int64_t* __restrict__ sizes,
                                                     const int64_t* __restrict__ offsets, uint8_t* __restrict__ dst)
{
    const int f = blockIdx.x;
    const uint8_t* s = slots + (long long)f * capacity;
    uint8_t* d = dst + offsets[f];
    const long long n = sizes[f];
    for (long long i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------------------------------------------------

LM_DEV uint32_t lm_get_be32(const uint8_t* p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// a wave per file: chunk walk, IHDR checks, IDAT payloads concatenated into zbuf[f]
__global__ void __launch_bounds__(64) lm_k_png_gather(const uint8_t* __restrict__ files, const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ lengths, int W, int H, uint8_t* __restrict__ zbuf, long long zcap,
                                                      int64_t* __restrict__ zlen, int32_t* __restrict__ status)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const uint8_t* p = files + offsets[f];
    const long long L = lengths[f];
    uint8_t* z = zbuf + (long long)f * zcap;
    int st = LM_PNG_OK;
    long long zn = 0;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (L < 8) st = LM_PNG_CORRUPT;
    for (int i = 0; i < 8 && st == LM_PNG_OK; i++)
        if (p[i] != sig[i]) st = LM_PNG_CORRUPT;
    long long pos = 8;
    bool have_ihdr = false, have_idat = false;
    while (st == LM_PNG_OK) {
        if (L - pos < 12) { st = LM_PNG_CORRUPT; break; }            // truncated before IEND
        const long long len = lm_get_be32(p + pos);
        const uint32_t tag = lm_get_be32(p + pos + 4);
        if (len > L - pos - 12) { st = LM_PNG_CORRUPT; break; }
        const uint8_t* body = p + pos + 8;
        if (!have_ihdr) {
            if (tag != 0x49484452u || len != 13) { st = LM_PNG_CORRUPT; break; }   // "IHDR" first
            have_ihdr = true;
            if (lm_get_be32(body) != (uint32_t)W || lm_get_be32(body + 4) != (uint32_t)H) { st = LM_PNG_CORRUPT; break; }
            if (body[10] != 0 || body[11] != 0) { st = LM_PNG_CORRUPT; break; }    // compression / filter method
            if (body[8] != 8 || body[9] != 0 || body[12] != 0) { st = LM_PNG_UNSUPPORTED; break; }
        } else if (tag == 0x49444154u) {                                           // "IDAT"
            have_idat = true;
            if (len > zcap - zn) { st = LM_PNG_UNSUPPORTED; break; }               // longer than the scratch: host decode
            for (long long i = lane; i < len; i += 64) z[zn + i] = body[i];
            zn += len;
        } else if (tag == 0x49454e44u) {                                           // "IEND"
            if (!have_idat) st = LM_PNG_CORRUPT;
            break;
        }
        pos += 12 + len;
    }
    if (lane == 0) {
        status[f] = st;
        zlen[f] = zn;
    }
}

#define LM_INF_WIN 4096            // LDS window of the compressed stream
#define LM_INF_RING 32768          // deflate window
#define LM_INF_CHUNK 8192          // ring flush granularity

struct LmHuff {
    int16_t count[16];
    int16_t symbol[288];
};

struct LmInflate {
    const uint8_t* z;               // compressed stream (global)
    long long zn;                   // its length
    long long ip;                   // next stream byte to load into bitbuf
    long long wbase;                // stream offset of win[0]
    unsigned long long bitbuf;
    int bitcnt;
    long long op;                   // output bytes produced
    long long flushed;              // output bytes copied to the raw scratch
    long long rawlen;
    uint8_t* raw;
    uint8_t* win;
    uint8_t* ring;
    int* flag;                      // LDS word for broadcasting lane 0's table checks
    int lane;
    bool bad;
};

// all lanes: the window is refilled cooperatively at the same (uniform) stream position
LM_DEV void lm_inf_window(LmInflate& s)
{
    __syncthreads();
    s.wbase = s.ip;
    for (int i = s.lane; i < LM_INF_WIN; i += 64) {
        const long long q = s.wbase + i;
        s.win[i] = q < s.zn ? s.z[q] : 0;
    }
    __syncthreads();
}

LM_DEV void lm_inf_refill(LmInflate& s)
{
    while (s.bitcnt <= 56 && s.ip < s.zn) {
        if (s.ip >= s.wbase + LM_INF_WIN) lm_inf_window(s);
        s.bitbuf |= (unsigned long long)s.win[s.ip - s.wbase] << s.bitcnt;
        s.bitcnt += 8;
        s.ip++;
    }
}

LM_DEV int lm_inf_bits(LmInflate& s, int n)
{
    if (s.bitcnt < n) lm_inf_refill(s);
    if (s.bitcnt < n) { s.bad = true; return 0; }
    const int v = (int)(s.bitbuf & ((1ull << n) - 1));
    s.bitbuf >>= n;
    s.bitcnt -= n;
    return v;
}

// canonical code decode (puff.c's decode): one bit at a time, at most 15
LM_DEV int lm_inf_decode(LmInflate& s, const LmHuff* h)
{
    if (s.bitcnt < 15) lm_inf_refill(s);
    int code = 0, first = 0, index = 0;
    unsigned long long buf = s.bitbuf;
    for (int len = 1; len <= 15; len++) {
        if (len > s.bitcnt) break;
        code |= (int)(buf & 1);
        buf >>= 1;
        const int count = h->count[len];
        if (code - count < first) {
            s.bitbuf >>= len;
            s.bitcnt -= len;
            return h->symbol[index + (code - first)];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    s.bad = true;       // out of data, or a code the table does not hold
    return 0;
}

// puff.c's construct, run by lane 0 between barriers: 0 = complete, > 0 incomplete, < 0 over-subscribed
LM_DEV int lm_inf_construct(LmHuff* h, const int16_t* length, int n)
{
    int16_t offs[16];
    for (int len = 0; len <= 15; len++) h->count[len] = 0;
    for (int sym = 0; sym < n; sym++) h->count[length[sym]]++;
    if (h->count[0] == n) return 0;
    int left = 1;
    for (int len = 1; len <= 15; len++) {
        left <<= 1;
        left -= h->count[len];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int len = 1; len < 15; len++) offs[len + 1] = offs[len] + h->count[len];
    for (int sym = 0; sym < n; sym++)
        if (length[sym] != 0) h->symbol[offs[length[sym]]++] = (int16_t)sym;
    return left;
}

// lane 0's verdict, seen by every lane
LM_DEV bool lm_inf_bcast(LmInflate& s, bool ok)
{
    __syncthreads();
    if (s.lane == 0) *s.flag = ok ? 1 : 0;
    __syncthreads();
    const bool r = *s.flag != 0;
    __syncthreads();
    return r;
}

// copies completed ring chunks (or, at the end, everything) to the raw scratch; all lanes
LM_DEV void lm_inf_flush(LmInflate& s, bool all)
{
    const long long upto = all ? s.op : (s.op / LM_INF_CHUNK) * LM_INF_CHUNK;
    if (upto <= s.flushed) return;
    __syncthreads();
    for (long long i = s.flushed + s.lane; i < upto; i += 64) s.raw[i] = s.ring[i & (LM_INF_RING - 1)];
    s.flushed = upto;
}

LM_DEV void lm_inf_literal(LmInflate& s, int v)
{
    if (s.op >= s.rawlen) { s.bad = true; return; }
    if (s.lane == 0) s.ring[s.op & (LM_INF_RING - 1)] = (uint8_t)v;
    s.op++;
    if ((s.op & (LM_INF_CHUNK - 1)) == 0) lm_inf_flush(s, false);
}

LM_DEV void lm_inf_match(LmInflate& s, int len, int dist)
{
    if (dist > s.op || s.op + len > s.rawlen) { s.bad = true; return; }
    __syncthreads();                       // literals and earlier copies visible to every lane
    for (int k = s.lane; k < len; k += 64)
        s.ring[(s.op + k) & (LM_INF_RING - 1)] = s.ring[(s.op - dist + (k % dist)) & (LM_INF_RING - 1)];
    __syncthreads();
    const long long before = s.op;
    s.op += len;
    if (s.op / LM_INF_CHUNK != before / LM_INF_CHUNK) lm_inf_flush(s, false);
}

LM_PNG_TABLE int16_t lm_inf_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
LM_PNG_TABLE int8_t lm_inf_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
LM_PNG_TABLE int16_t lm_inf_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                                      4097, 6145, 8193, 12289, 16385, 24577};
LM_PNG_TABLE int8_t lm_inf_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
LM_PNG_TABLE int8_t lm_inf_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

LM_DEV void lm_inf_codes(LmInflate& s, const LmHuff* lc, const LmHuff* dc)
{
    for (;;) {
        const int sym = lm_inf_decode(s, lc);
        if (s.bad) return;
        if (sym < 256) { lm_inf_literal(s, sym); if (s.bad) return; continue; }
        if (sym == 256) return;
        const int li = sym - 257;
        if (li >= 29) { s.bad = true; return; }
        const int len = lm_inf_lbase[li] + lm_inf_bits(s, lm_inf_lext[li]);
        const int ds = lm_inf_decode(s, dc);
        if (s.bad) return;
        if (ds >= 30) { s.bad = true; return; }
        const int dist = lm_inf_dbase[ds] + lm_inf_bits(s, lm_inf_dext[ds]);
        if (s.bad) return;
        lm_inf_match(s, len, dist);
        if (s.bad) return;
    }
}

// a wave per file: zlib stream in zbuf[f] -> the raw (filtered) rows in raw[f]; the stream's adler32 -> adler[f]
__global__ void __launch_bounds__(64) lm_k_png_inflate(const uint8_t* __restrict__ zbuf, long long zcap, const int64_t* __restrict__ zlen,
                                                       uint8_t* __restrict__ rawbuf, long long rawcap, long long rawlen, uint32_t* __restrict__ adler,
                                                       int32_t* __restrict__ status)
{
    __shared__ uint8_t s_win[LM_INF_WIN];
    __shared__ uint8_t s_ring[LM_INF_RING];
    __shared__ LmHuff s_lc, s_dc;
    __shared__ int16_t s_len[288 + 32];
    __shared__ int s_flag;
    const int f = blockIdx.x;
    if (status[f] != LM_PNG_OK) return;
    LmInflate s;
    s.z = zbuf + (long long)f * zcap;
    s.zn = zlen[f];
    s.ip = 0;
    s.wbase = 0;
    s.bitbuf = 0;
    s.bitcnt = 0;
    s.op = 0;
    s.flushed = 0;
    s.rawlen = rawlen;
    s.raw = rawbuf + (long long)f * rawcap;
    s.win = s_win;
    s.ring = s_ring;
    s.flag = &s_flag;
    s.lane = threadIdx.x;
    s.bad = false;
    lm_inf_window(s);
    const int cmf = lm_inf_bits(s, 8), flg = lm_inf_bits(s, 8);
    if (s.bad || (cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) s.bad = true;
    int last = 0;
    while (!s.bad && !last) {
        last = lm_inf_bits(s, 1);
        const int type = lm_inf_bits(s, 2);
        if (s.bad) break;
        if (type == 0) {                                     // stored
            s.bitbuf >>= (s.bitcnt & 7);
            s.bitcnt -= (s.bitcnt & 7);
            const int len = lm_inf_bits(s, 16), nlen = lm_inf_bits(s, 16);
            if (s.bad || len != (~nlen & 0xffff)) { s.bad = true; break; }
            for (int i = 0; i < len && !s.bad; i++) {
                const int v = lm_inf_bits(s, 8);
                if (!s.bad) lm_inf_literal(s, v);
            }
        } else if (type == 1 || type == 2) {
            __syncthreads();                                 // every lane is done with the previous block's tables
            bool ok = true;
            if (type == 1) {
                if (s.lane == 0) {
                    int sym = 0;
                    for (; sym < 144; sym++) s_len[sym] = 8;
                    for (; sym < 256; sym++) s_len[sym] = 9;
                    for (; sym < 280; sym++) s_len[sym] = 7;
                    for (; sym < 288; sym++) s_len[sym] = 8;
                    lm_inf_construct(&s_lc, s_len, 288);
                    for (sym = 0; sym < 30; sym++) s_len[sym] = 5;
                    lm_inf_construct(&s_dc, s_len, 30);
                }
            } else {
                const int nlen = lm_inf_bits(s, 5) + 257, ndist = lm_inf_bits(s, 5) + 1, ncode = lm_inf_bits(s, 4) + 4;
                if (s.bad || nlen > 286 || ndist > 30) { s.bad = true; break; }
                int16_t cl[19];
                for (int i = 0; i < 19; i++) cl[i] = 0;
                for (int i = 0; i < ncode; i++) cl[lm_inf_clorder[i]] = (int16_t)lm_inf_bits(s, 3);
                if (s.bad) break;
                if (s.lane == 0) ok = lm_inf_construct(&s_lc, cl, 19) == 0;
                if (!lm_inf_bcast(s, ok)) { s.bad = true; break; }
                int idx = 0;
                while (idx < nlen + ndist && !s.bad) {
                    int sym = lm_inf_decode(s, &s_lc);
                    if (s.bad) break;
                    if (sym < 16) { if (s.lane == 0) s_len[idx] = (int16_t)sym; idx++; continue; }
                    int prev = 0, rep;
                    if (sym == 16) {
                        if (idx == 0) { s.bad = true; break; }
                        __syncthreads();
                        prev = s_len[idx - 1];
                        __syncthreads();
                        rep = 3 + lm_inf_bits(s, 2);
                    } else if (sym == 17) rep = 3 + lm_inf_bits(s, 3);
                    else rep = 11 + lm_inf_bits(s, 7);
                    if (s.bad || idx + rep > nlen + ndist) { s.bad = true; break; }
                    for (; rep > 0; rep--, idx++) if (s.lane == 0) s_len[idx] = (int16_t)prev;
                }
                if (s.bad) break;
                __syncthreads();
                if (s.lane == 0) {
                    if (s_len[256] == 0) ok = false;
                    const int e1 = lm_inf_construct(&s_lc, s_len, nlen);
                    if (e1 < 0 || (e1 > 0 && nlen - s_lc.count[0] != 1)) ok = false;      // incomplete only for a single code
                    const int e2 = lm_inf_construct(&s_dc, s_len + nlen, ndist);
                    if (e2 < 0 || (e2 > 0 && ndist - s_dc.count[0] != 1)) ok = false;
                }
            }
            if (!lm_inf_bcast(s, ok)) { s.bad = true; break; }
            lm_inf_codes(s, &s_lc, &s_dc);
        } else {
            s.bad = true;
        }
    }
    if (!s.bad && s.op != s.rawlen) s.bad = true;
    uint32_t ad = 0;
    if (!s.bad) {
        s.bitbuf >>= (s.bitcnt & 7);
        s.bitcnt -= (s.bitcnt & 7);
        for (int i = 0; i < 4 && !s.bad; i++) ad = (ad << 8) | (uint32_t)lm_inf_bits(s, 8);
    }
    if (!s.bad) lm_inf_flush(s, true);
    if (s.lane == 0) {
        if (s.bad) status[f] = LM_PNG_CORRUPT;
        else adler[f] = ad;
    }
}

LM_DEV int lm_paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

#define LM_UNF_T 256
// a block per frame: the five row filters undone row by row (previous row kept in LDS) + the adler32 check
__global__ void __launch_bounds__(LM_UNF_T) lm_k_png_unfilter(const uint8_t* __restrict__ rawbuf, long long rawcap, int W, int H,
                                                              const uint32_t* __restrict__ adler, uint8_t* __restrict__ frames,
                                                              int32_t* __restrict__ status)
{
    LM_DYN_SMEM(smem);
    __shared__ unsigned long long s_a[LM_UNF_T], s_b[LM_UNF_T];
    const int f = blockIdx.x, t = threadIdx.x;
    if (status[f] != LM_PNG_OK) return;
    uint8_t* prev = (uint8_t*)smem;
    uint8_t* cur = prev + W;
    const uint8_t* raw = rawbuf + (long long)f * rawcap;
    uint8_t* out = frames + (long long)f * W * H;
    const unsigned long long total = (unsigned long long)(W + 1) * H;
    unsigned long long a = 0, b = 0;
    for (int x = t; x < W; x += LM_UNF_T) prev[x] = 0;
    for (int y = 0; y < H; y++) {
        const uint8_t* r = raw + (long long)y * (W + 1);
        const int ft = r[0];
        if (t == 0) {
            a += ft;
            b += (unsigned long long)((total - (unsigned long long)y * (W + 1)) % LM_PNG_ADLER) * ft;
        }
        for (int x = t; x < W; x += LM_UNF_T) {
            const unsigned d = r[1 + x];
            a += d;
            b += (unsigned long long)((total - (unsigned long long)y * (W + 1) - 1 - x) % LM_PNG_ADLER) * d;
            cur[x] = (uint8_t)d;
        }
        __syncthreads();             // cur holds the filtered row; prev the previous output row
        if (ft == 0 || ft == 2) {
            if (ft == 2)
                for (int x = t; x < W; x += LM_UNF_T) cur[x] = (uint8_t)(cur[x] + prev[x]);
        } else if (ft <= 4) {
            if (t == 0) {
                int left = 0, ul = 0;
                for (int x = 0; x < W; x++) {
                    const int up = prev[x];
                    int v = cur[x];
                    if (ft == 1) v += left;
                    else if (ft == 3) v += (left + up) >> 1;
                    else v += lm_paeth(left, up, ul);
                    left = v & 255;
                    ul = up;
                    cur[x] = (uint8_t)left;
                }
            }
        }
        __syncthreads();
        if (ft > 4) {                // uniform: every thread read the same filter byte
            if (t == 0) status[f] = LM_PNG_CORRUPT;
            return;
        }
        for (int x = t; x < W; x += LM_UNF_T) out[(long long)y * W + x] = cur[x];
        uint8_t* tmp = prev;
        prev = cur;
        cur = tmp;
        __syncthreads();
    }
    s_a[t] = a % LM_PNG_ADLER;
    s_b[t] = b % LM_PNG_ADLER;
    __syncthreads();
    if (t == 0) {
        unsigned long long A = 1, B = total % LM_PNG_ADLER;
        for (int i = 0; i < LM_UNF_T; i++) { A += s_a[i]; B += s_b[i]; }
        A %= LM_PNG_ADLER;
        B %= LM_PNG_ADLER;
        if ((uint32_t)((B << 16) | A) != adler[f]) status[f] = LM_PNG_CORRUPT;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------

struct LmPng {
    int W, H, max_batch;
    // encoder scratch (allocated on first use)
    uint32_t* rowbits = nullptr;
    uint32_t* rowoff = nullptr;
    uint32_t* adl = nullptr;
    uint32_t* dbytes = nullptr;
    // decoder scratch (allocated on first use)
    uint8_t* zbuf = nullptr;
    long long zcap = 0;
    int64_t* zlen = nullptr;
    uint8_t* raw = nullptr;
    long long rawcap = 0;
    uint32_t* adler = nullptr;
};

extern "C" int64_t lm_png_encode_bound(int width, int height)
{
    if (width <= 0 || height <= 0) return 0;
    const long long bits = 10 + 9 * lm_png_raw_bytes(width, height);
    return ((LM_PNG_HEAD + (bits + 7) / 8 + LM_PNG_TAIL) + 15) / 16 * 16;
}

extern "C" void lm_png_destroy(LmPng* p)
{
    if (!p) return;
    (void)hipFree(p->rowbits);
    (void)hipFree(p->rowoff);
    (void)hipFree(p->adl);
    (void)hipFree(p->dbytes);
    (void)hipFree(p->zbuf);
    (void)hipFree(p->zlen);
    (void)hipFree(p->raw);
    (void)hipFree(p->adler);
    delete p;
}

extern "C" LmPng* lm_png_create(int width, int height, int max_batch)
{
    // every frame's deflate bits must fit the 32-bit row offsets: 9 * H * (W + 1) + 10 < 2^32
    if (width <= 0 || height <= 0 || width > LM_PNG_MAX_W || max_batch <= 0 || max_batch > 1024 ||
        lm_png_raw_bytes(width, height) > 400000000ll) {
        lm_set_error("lm_png_create: bad arguments (width=%d height=%d max_batch=%d; width <= %d, height * (width + 1) <= 4e8, batch <= 1024)", width,
                     height, max_batch, LM_PNG_MAX_W);
        return nullptr;
    }
    LmPng* p = new LmPng();
    p->W = width;
    p->H = height;
    p->max_batch = max_batch;
    return p;
}

static int lm_png_alloc(void** ptr, size_t bytes)
{
    if (*ptr) return LM_OK;
    if (hipMalloc(ptr, bytes) != hipSuccess) {
        *ptr = nullptr;
        lm_set_error("lm_png: hipMalloc of %zu bytes failed", bytes);
        return LM_ERR_HIP;
    }
    return LM_OK;
}

extern "C" int lm_png_encode(LmPng* p, const uint8_t* d_frames, int n, uint8_t* d_out, int64_t capacity, int64_t* d_sizes, void* stream)
{
    if (!p || !d_frames || !d_out || !d_sizes || n < 0 || n > (p ? p->max_batch : 0) || capacity < lm_png_encode_bound(p->W, p->H) || (capacity & 3) ||
        ((uintptr_t)d_out & 3)) {
        lm_set_error("lm_png_encode: bad arguments (n=%d, capacity=%lld, bound=%lld, output 4-byte aligned)", n, capacity,
                     p ? lm_png_encode_bound(p->W, p->H) : 0ll);
        return LM_ERR_ARG;
    }
    if (n == 0) return LM_OK;
    const size_t rows = (size_t)p->max_batch * p->H;
    int rc = lm_png_alloc((void**)&p->rowbits, rows * 4);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->rowoff, rows * 4);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->adl, rows * 8);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->dbytes, (size_t)p->max_batch * 4);
    if (rc != LM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long nr = (long long)n * p->H;
    const unsigned blocks = (unsigned)((nr + 255) / 256);
    hipLaunchKernelGGL(lm_k_png_rows<0>, dim3(blocks), dim3(256), 0, st, d_frames, p->W, p->H, n, p->rowbits, p->adl, (const uint32_t*)nullptr,
                       (uint8_t*)nullptr, capacity);
    hipLaunchKernelGGL(lm_k_png_frame, dim3(n), dim3(LM_PNG_FT), 0, st, p->W, p->H, p->rowbits, p->adl, p->rowoff, d_out, capacity, d_sizes, p->dbytes);
    hipLaunchKernelGGL(lm_k_png_rows<1>, dim3(blocks), dim3(256), 0, st, d_frames, p->W, p->H, n, (uint32_t*)nullptr, (uint32_t*)nullptr, p->rowoff,
                       d_out, capacity);
    hipLaunchKernelGGL(lm_k_png_crc, dim3(n), dim3(LM_PNG_FT), 0, st, d_out, capacity, p->dbytes);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_png_pack(const uint8_t* d_slots, int64_t capacity, const int64_t* d_sizes, const int64_t* d_offsets, int n, uint8_t* d_dst, void* stream)
{
    if (!d_slots || !d_sizes || !d_offsets || !d_dst || n < 0 || capacity <= 0) {
        lm_set_error("lm_png_pack: bad arguments");
        return LM_ERR_ARG;
    }
    if (n == 0) return LM_OK;
    hipLaunchKernelGGL(lm_k_png_pack, dim3(n), dim3(256), 0, (hipStream_t)stream, d_slots, capacity, d_sizes, d_offsets, d_dst);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

extern "C" int lm_png_decode(LmPng* p, const uint8_t* d_files, const int64_t* d_offsets, const int64_t* d_lengths, int n, uint8_t* d_frames,
                             int32_t* d_status, void* stream)
{
    if (!p || !d_files || !d_offsets || !d_lengths || !d_frames || !d_status || n < 0 || n > p->max_batch) {
        lm_set_error("lm_png_decode: bad arguments (n=%d, max_batch=%d)", n, p ? p->max_batch : 0);
        return LM_ERR_ARG;
    }
    if (n == 0) return LM_OK;
    const long long rawlen = lm_png_raw_bytes(p->W, p->H);
    if (!p->raw) {
        p->rawcap = (rawlen + 15) / 16 * 16;
        p->zcap = (rawlen + rawlen / 8 + 4096 + 15) / 16 * 16;   // stored blocks or 9-bit literals fit; anything longer goes to the host
    }
    int rc = lm_png_alloc((void**)&p->raw, (size_t)p->rawcap * p->max_batch);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->zbuf, (size_t)p->zcap * p->max_batch);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->zlen, (size_t)p->max_batch * 8);
    if (rc == LM_OK) rc = lm_png_alloc((void**)&p->adler, (size_t)p->max_batch * 4);
    if (rc != LM_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lm_k_png_gather, dim3(n), dim3(64), 0, st, d_files, d_offsets, d_lengths, p->W, p->H, p->zbuf, p->zcap, p->zlen, d_status);
    hipLaunchKernelGGL(lm_k_png_inflate, dim3(n), dim3(64), 0, st, p->zbuf, p->zcap, p->zlen, p->raw, p->rawcap, rawlen, p->adler, d_status);
    hipLaunchKernelGGL(lm_k_png_unfilter, dim3(n), dim3(LM_UNF_T), (size_t)2 * p->W, st, p->raw, p->rawcap, p->W, p->H, p->adler, d_frames, d_status);
    LM_HIP(hipGetLastError());
    return LM_OK;
}
