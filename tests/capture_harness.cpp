// capture_harness.cpp -- a stand-alone reader over the capture source's public C ABI (include/evcap.h), meant to be built
// with -fsanitize=address,undefined together with the eight sources of evenvizion_amd/capture/ (not against libevcap.so)
// and started as a child process by tests/test_capture_hostile.py.
//
//     capture_harness FILE [MAX_FRAMES]     decode FILE, at most MAX_FRAMES frames (default: all)
//     capture_harness --selftest-overread   read one byte past a heap block (the sanitizer must report it)
//
// Output, one line each:
//     INFO w=<w> h=<h> n=<samples> fps=<fps>
//     FRAME <i> bgr|yuv <sha256> poc=<poc> idx=<decode index> type=<0 P|1 B|2 I>
//                                   even i: read_bgr, the digest of the BGR rows; odd i: read_yuv420, the digest of Y, Cb, Cr
//     REFUSED <i> yuv code=<n>      read_yuv420 refused its arguments (odd crop offset); the frame is then read as BGR
//     STATS <the counters of evcap_stats>
//     LAST poc=<poc> idx=<decode index> type=<0 P|1 B|2 I>  |  LAST none
//     INFO ...                      evcap_info again, after the last read
//     END frames=<k>  |  ERR code=<n> msg=<text>             always the last line
// The exit status is 0 in every one of these cases.  Anything else (a sanitizer report, a signal, an exception that
// crossed the ABI) ends the process with another status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/evcap.h"

namespace {

struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t buf[64];
    uint64_t total = 0;
    size_t fill = 0;
    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t* p) {
        static const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
            0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
            0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
            0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
            0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
            0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
            0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t(p[4 * i]) << 24) | (uint32_t(p[4 * i + 1]) << 16) | (uint32_t(p[4 * i + 2]) << 8) | uint32_t(p[4 * i + 3]);
        for (int i = 16; i < 64; ++i) {
            uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const uint8_t* p, size_t n) {
        total += n;
        while (n) {
            size_t k = 64 - fill < n ? 64 - fill : n;
            std::memcpy(buf + fill, p, k);
            fill += k; p += k; n -= k;
            if (fill == 64) {
                block(buf);
                fill = 0;
            }
        }
    }
    std::string hex() {
        uint64_t bits = total * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while (fill != 56) update(&zero, 1);
        uint8_t len[8];
        for (int i = 0; i < 8; ++i) len[i] = uint8_t(bits >> (56 - 8 * i));
        update(len, 8);
        char out[65];
        for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
        return std::string(out, 64);
    }
};

void print_info(evcap* c) {
    int w = 0, h = 0, n = 0;
    double fps = 0;
    evcap_info(c, &w, &h, &n, &fps);
    std::printf("INFO w=%d h=%d n=%d fps=%.6f\n", w, h, n, fps);
}

// the message on one line
std::string one_line(const char* s) {
    std::string o(s ? s : "");
    for (char& ch : o)
        if (ch == '\n' || ch == '\r') ch = ' ';
    return o;
}

int selftest_overread() {
    volatile size_t size = 16;  // volatile: the compiler must not know the block's size, the run-time check has to find it
    volatile uint8_t* p = (volatile uint8_t*)std::malloc(size);
    for (int i = 0; i < 16; ++i) p[i] = (uint8_t)i;
    volatile int past = 16;
    std::printf("SELFTEST read %d\n", (int)p[past]);  // one byte past the block
    std::free((void*)p);
    std::printf("SELFTEST the overread was not reported\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "--selftest-overread") == 0) return selftest_overread();
    if (argc < 2) {
        std::fprintf(stderr, "usage: capture_harness FILE [MAX_FRAMES] | --selftest-overread\n");
        return 2;
    }
    long limit = argc >= 3 ? std::atol(argv[2]) : -1;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (sz < 0) sz = 0;
    uint8_t* file = (uint8_t*)std::malloc(sz ? (size_t)sz : 1);  // exactly the file: an overread by the demultiplexer is seen
    if (sz && std::fread(file, 1, (size_t)sz, f) != (size_t)sz) {
        std::fprintf(stderr, "short read on %s\n", argv[1]);
        return 2;
    }
    std::fclose(f);

    evcap* c = nullptr;
    int rc = evcap_open_memory(file, (uint64_t)sz, &c);
    std::free(file);  // the ABI says the buffer is copied
    if (rc != EVCAP_OK || !c) {
        std::printf("ERR code=%d msg=%s\n", rc, one_line(evcap_last_error(nullptr)).c_str());
        return 0;
    }
    print_info(c);
    int w = 0, h = 0;
    evcap_info(c, &w, &h, nullptr, nullptr);
    const size_t cw = (size_t)(w + 1) / 2, ch = (size_t)(h + 1) / 2;
    long frames = 0;
    std::string final_line;
    bool yuv_refused = false;
    for (;;) {
        if (limit >= 0 && frames >= limit) break;
        bool as_yuv = (frames & 1) && !yuv_refused;
        Sha256 sha;
        if (as_yuv) {
            uint8_t* y = (uint8_t*)std::malloc((size_t)w * h);
            uint8_t* cb = (uint8_t*)std::malloc(cw * ch);
            uint8_t* cr = (uint8_t*)std::malloc(cw * ch);
            rc = evcap_read_yuv420(c, y, w, cb, cr, (int64_t)cw);
            if (rc == EVCAP_OK) {
                sha.update(y, (size_t)w * h);
                sha.update(cb, cw * ch);
                sha.update(cr, cw * ch);
            }
            std::free(y);
            std::free(cb);
            std::free(cr);
            if (rc == EVCAP_ERR_INVALID) {  // refused before a picture was taken: the frame is still there
                std::printf("REFUSED %ld yuv code=%d\n", frames, rc);
                yuv_refused = true;
                continue;
            }
        } else {
            uint8_t* bgr = (uint8_t*)std::malloc((size_t)w * h * 3);
            rc = evcap_read_bgr(c, bgr, (int64_t)w * 3);
            if (rc == EVCAP_OK) sha.update(bgr, (size_t)w * h * 3);
            std::free(bgr);
        }
        if (rc == EVCAP_EOF) break;
        if (rc != EVCAP_OK) {
            final_line = "ERR code=" + std::to_string(rc) + " msg=" + one_line(evcap_last_error(c));
            break;
        }
        int poc = 0, idx = 0, type = 0;
        evcap_last_frame_info(c, &poc, &idx, &type);
        std::printf("FRAME %ld %s %s poc=%d idx=%d type=%d\n", frames, as_yuv ? "yuv" : "bgr", sha.hex().c_str(), poc, idx, type);
        ++frames;
    }
    int64_t st[64];
    int ns = evcap_stats(c, st, 64);
    std::printf("STATS");
    for (int i = 0; i < ns && i < 64; ++i) std::printf(" %lld", (long long)st[i]);
    std::printf("\n");
    int poc = 0, idx = 0, type = 0;
    if (evcap_last_frame_info(c, &poc, &idx, &type) == EVCAP_OK)
        std::printf("LAST poc=%d idx=%d type=%d\n", poc, idx, type);
    else
        std::printf("LAST none\n");
    print_info(c);
    evcap_close(c);
    if (final_line.empty()) final_line = "END frames=" + std::to_string(frames);
    std::printf("%s\n", final_line.c_str());
    return 0;
}
