// TEST INFRASTRUCTURE ONLY -- runs the host build of transformerupscaler_amd/csrc/png_deflate.h, the code the GPU PNG encoder runs for
// its Huffman codes, header run lengths and checksums.  tests/test_png_cpu.py builds it with the address and undefined-behaviour
// sanitizers and compares what it prints with tests/_png_ref.py.
//
// Input file: one command a line, numbers separated by blanks.
//   L <limit> <nsym> <count>...      -> "L <length>... | <code>..."           code lengths and canonical codes (bits reversed)
//   R <n> <length>...                -> "R <token>... | <cl count>..."        tokens as symbol | value << 8
//   C <piece> <n> <byte>...          -> "C <crc32>"                           from pieces of <piece> bytes combined
//   A <block> <n> <byte>...          -> "A <adler32>"                         from per-block partials combined
//   S <from> <to>                    -> "S <symbol,extra,value>..."           match lengths from..to
//   F                                -> "F <code>..."                         the fixed literal / length code, 288 codes (bits reversed)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "png_deflate.h"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd;
    while (fscanf(f, " %c", &cmd) == 1) {
        if (cmd == 'L') {
            int limit, nsym;
            if (fscanf(f, "%d %d", &limit, &nsym) != 2 || nsym < 1 || nsym > PD_LIT || limit < 1 || limit > 15) return 2;
            // exactly the sizes the builder may touch: a write past them is an error the sanitizer sees
            std::vector<int> freq(nsym), sorted(nsym), count(16);
            std::vector<uint16_t> order(nsym);
            std::vector<uint8_t> lens(nsym);
            for (int i = 0; i < nsym; ++i)
                if (fscanf(f, "%d", &freq[i]) != 1) return 2;
            pd_build_lengths(freq.data(), nsym, limit, sorted.data(), order.data(), count.data(), lens.data());
            printf("L");
            for (int i = 0; i < nsym; ++i) printf(" %d", lens[i]);
            printf(" |");
            for (int i = 0; i < nsym; ++i) printf(" %u", pd_code(lens.data(), nsym, i));
            printf("\n");
        } else if (cmd == 'R') {
            int n;
            if (fscanf(f, "%d", &n) != 1 || n < 1 || n > PD_MAX_SEQ) return 2;
            std::vector<uint8_t> seq(n);
            std::vector<uint16_t> tokens(n);
            std::vector<int> cl(PD_CL);
            for (int i = 0, v; i < n; ++i) {
                if (fscanf(f, "%d", &v) != 1 || v < 0 || v > 15) return 2;
                seq[i] = (uint8_t)v;
            }
            const int nt = pd_run_length_code(seq.data(), n, tokens.data(), cl.data());
            printf("R");
            for (int i = 0; i < nt; ++i) printf(" %d", tokens[i]);
            printf(" |");
            for (int i = 0; i < PD_CL; ++i) printf(" %d", cl[i]);
            printf("\n");
        } else if (cmd == 'C' || cmd == 'A') {
            int piece, n;
            if (fscanf(f, "%d %d", &piece, &n) != 2 || piece < 1 || n < 0) return 2;
            std::vector<uint8_t> d(n);
            for (int i = 0, v; i < n; ++i) {
                if (fscanf(f, "%d", &v) != 1) return 2;
                d[i] = (uint8_t)v;
            }
            if (cmd == 'C') {
                uint32_t acc = 0;
                for (int p0 = 0; p0 < n; p0 += piece) {
                    const int p1 = p0 + piece < n ? p0 + piece : n;
                    uint32_t s = 0;
                    for (int i = p0; i < p1; ++i) s = pd_crc_byte(s, d[i]);
                    acc ^= pd_crc_mul(s, pd_crc_shift((uint32_t)(n - p1)));
                }
                printf("C %u\n", pd_crc_finish(acc, (uint32_t)n));
            } else {
                uint32_t A = 1, B = 0;
                for (int p0 = 0; p0 < n; p0 += piece) {
                    const int p1 = p0 + piece < n ? p0 + piece : n;
                    uint64_t a = 0, b = 0;
                    for (int i = p0; i < p1; ++i) { a += d[i]; b += (uint64_t)(p1 - i) * d[i]; }
                    pd_adler_append(A, B, (uint32_t)(b % PD_ADLER) << 16 | (uint32_t)(a % PD_ADLER), (uint32_t)(p1 - p0));
                }
                printf("A %u\n", B << 16 | A);
            }
        } else if (cmd == 'S') {
            int from, to;
            if (fscanf(f, "%d %d", &from, &to) != 2 || from < 3 || to > 258) return 2;
            printf("S");
            for (int len = from; len <= to; ++len) {
                int extra, value;
                const int sym = pd_length_symbol(len, extra, value);
                if (pd_length_extra(sym) != extra) return 3;
                printf(" %d,%d,%d", sym, extra, value);
            }
            printf("\n");
        } else if (cmd == 'F') {
            std::vector<uint8_t> lens(288);
            for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)pd_fixed_length(i);
            printf("F");
            for (int i = 0; i < 288; ++i) printf(" %u", pd_code(lens.data(), 288, i));
            printf("\n");
        } else {
            return 2;
        }
    }
    fclose(f);
    return 0;
}
