// csrc/png_inflate.h on the host: the walker the inflate kernel runs, one lane wide, with every stream and every output in a heap block
// of exactly its size, so that the address sanitizer sees any byte read or written outside them (tests/test_png_decode_cpu.py builds
// this with -fsanitize=address,undefined and runs it as a child process).  Input: a file of lines
//   I <total> <stream as hex>            -> "<status> <crc32 of the total output bytes, zeros where nothing was written>"
//   U <H> <W> <bpp> <filtered as hex>    -> "<a filter byte was above 4> <crc32 of the H * W * bpp reconstructed bytes>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "png_inflate.h"

namespace {
struct HostSrc {
    const uint8_t* data;
    uint64_t n;
    uint64_t nbits() const { return 8 * n; }
    uint64_t peek(uint64_t pos) const
    {
        const uint64_t byte = pos >> 3;
        const int s = (int)(pos & 7);
        uint64_t w = 0;
        for (int k = 0; k < 8; ++k)
            if (byte + k < n) w |= (uint64_t)data[byte + k] << (8 * k);
        w >>= s;
        if (s && byte + 8 < n) w |= (uint64_t)data[byte + 8] << (64 - s);
        return w;
    }
};

struct HostSink {
    uint8_t* out;
    const uint8_t* in;
    uint32_t total;
    void lit(uint32_t o, int v) { out[o] = (uint8_t)v; }
    void match(uint32_t o, int len, int dist)
    {
        for (int k = 0; k < len; ++k) out[o + k] = out[o - dist + k % dist];
    }
    void stored(uint32_t o, uint64_t byte, uint32_t n) { memcpy(out + o, in + byte, n); }
    void advance(uint32_t) {}
    uint32_t finish(uint32_t o) const
    {
        uint32_t A = 1, B = 0;
        for (uint32_t i = 0; i < o; ++i) { A = (A + out[i]) % PD_ADLER; B = (B + A) % PD_ADLER; }
        return B << 16 | A;
    }
};

uint32_t crc(const uint8_t* p, size_t n)
{
    uint32_t s = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) s = pd_crc_byte(s, p[i]);
    return s ^ 0xFFFFFFFFu;
}

uint8_t* unhex(const std::string& h, size_t& n)
{
    n = h == "-" ? 0 : h.size() / 2;
    uint8_t* p = new uint8_t[n];
    for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    return p;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    PiTables* t = new PiTables;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string kind, hex;
        is >> kind;
        if (kind == "I") {
            uint32_t total;
            is >> total >> hex;
            size_t n;
            uint8_t* in = unhex(hex, n);
            uint8_t* out = new uint8_t[total]();
            HostSrc src = {in, n};
            HostSink sink = {out, in, total};
            const int st = pi_inflate(*t, src, sink, PiTokenWalk(), total, 0, 1);
            printf("%d %u\n", st, crc(out, total));
            delete[] in;
            delete[] out;
        } else if (kind == "U") {
            int H, W, bpp;
            is >> H >> W >> bpp >> hex;
            size_t n;
            uint8_t* in = unhex(hex, n);
            const size_t row = (size_t)W * bpp;
            if (n != (size_t)H * (1 + row)) return 3;
            uint8_t* out = new uint8_t[H * row];
            int bad = 0;
            for (int y = 0; y < H; ++y) {
                int ft = in[y * (1 + row)];
                if (ft > 4) { bad = 1; ft = 0; }
                for (size_t i = 0; i < row; ++i) {
                    const int a = i >= (size_t)bpp ? out[y * row + i - bpp] : 0, b = y ? out[(y - 1) * row + i] : 0;
                    const int c = y && i >= (size_t)bpp ? out[(y - 1) * row + i - bpp] : 0;
                    out[y * row + i] = (uint8_t)pi_unfilter_byte(ft, in[y * (1 + row) + 1 + i], a, b, c);
                }
            }
            printf("%d %u\n", bad, crc(out, H * row));
            delete[] in;
            delete[] out;
        } else if (!kind.empty()) return 4;
    }
    delete t;
    return 0;
}
