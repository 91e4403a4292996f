// Host driver of the decode engine's LoRA-2 pack (web-rwkv-gguf_amd/csrc/wrk_lora2_pack.h): packs four synthetic F16 matrices with
// eng_l2_pack_layer and then reads the image back the way a head workgroup of v7_engine_kernel does -- piece (head, u, n) at the offset
// the kernel computes, lane L's 16 bytes into register n -- against the register contents of the kernel BEFORE the pack, which are
// restated here from the matrices themselves and not through the header's source functions.  One JSON line per case.
// Built and run by tests/test_engine_lora2_pack_host.py, which holds the expectations.
//
// A case is one line:  name H rw ra rg rv has_v row_pad dump
//   has_v   0: no fourth matrix (layer 0)        row_pad: bytes between the rows of a matrix beyond rank * 2 (a multiple of 16)
//   dump    1: the whole image follows as hex in "image"
// Element (m, row, col) of the source is the odd 16-bit word elem(m, row, col): never zero, so a padding lane is told from data.
#include "wrk_lora2_pack.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace wrk;

static uint16_t elem(uint32_t m, uint32_t row, uint32_t col) { return (uint16_t)(((m * 7919u + row * 131u + col * 17u) << 1) | 1u); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream cs(line);
        std::string name;
        uint32_t H = 0, rk[4] = {0, 0, 0, 0}, has_v = 1, row_pad = 0, dump = 0;
        cs >> name >> H >> rk[0] >> rk[1] >> rk[2] >> rk[3] >> has_v >> row_pad >> dump;
        if (!cs || H == 0) { fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        const EngLora2Ranks R{rk[0], rk[1], rk[2], rk[3]};
        const uint32_t rows = H * 64u;
        // the matrices, each in an allocation of exactly its size (the sanitizer sees a read past a row or a matrix)
        std::vector<std::vector<uint8_t>> mat(4);
        const uint8_t* src[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t rb[4] = {0, 0, 0, 0};
        for (uint32_t m = 0; m < 4; ++m) {
            if (m == 3 && !has_v) continue;
            rb[m] = (size_t)rk[m] * 2 + row_pad;
            mat[m].assign((size_t)rows * rb[m], 0xEE);          // the bytes between rows are never copied: 0xEE in the image is an error
            for (uint32_t r = 0; r < rows; ++r)
                for (uint32_t c = 0; c < rk[m]; ++c) { const uint16_t v = elem(m, r, c); memcpy(&mat[m][(size_t)r * rb[m] + 2u * c], &v, 2); }
            src[m] = mat[m].data();
        }
        const size_t bytes = eng_l2_layer_bytes(R, H);
        std::vector<uint8_t> img(bytes);
        eng_l2_pack_layer(R, H, src, rb, img.data());

        // read back as the kernel does
        std::vector<std::vector<uint8_t>> seen(4);
        for (uint32_t m = 0; m < 4; ++m) seen[m].assign((size_t)rows * rk[m], 0);
        std::vector<uint8_t> piece_used(bytes / ENG_L2_PIECE_BYTES, 0);
        uint64_t mismatches = 0, pad_nonzero = 0, beyond_rank = 0, misaligned = 0, out_of_image = 0, twice = 0, pad_lanes = 0;
        for (uint32_t head = 0; head < H; ++head)
            for (uint32_t u = 0; u < 16; ++u) {
                const uint32_t mi = u >> 2, bi = u & 3u;
                for (uint32_t n = 0; n < eng_l2_pieces(rk[mi]); ++n) {
                    if (32u * n >= rk[mi]) ++beyond_rank;
                    const size_t off = eng_l2_piece(R, head, u, n) * ENG_L2_PIECE_BYTES;
                    if (off % 1024u) ++misaligned;
                    if (off + 1024u > bytes) { ++out_of_image; continue; }
                    if (piece_used[off / 1024u]++) ++twice;
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        // the parent kernel: row c0 + 16 bi + (lane >> 2), columns (lane & 3) * 8 + 32 n .. + 8 of matrix mi into lu[i][n]
                        const uint32_t row = head * 64u + 16u * bi + (lane >> 2), c = (lane & 3u) * 8u + 32u * n;
                        uint16_t reg[8];
                        memcpy(reg, &img[off + 16u * lane], 16);
                        if (c >= rk[mi]) { ++pad_lanes; for (int e = 0; e < 8; ++e) pad_nonzero += reg[e] != 0; continue; }   // eng_lora_dot never reads it
                        for (uint32_t e = 0; e < 8; ++e) {
                            const uint16_t want = (mi == 3 && !has_v) ? 0 : elem(mi, row, c + e);
                            mismatches += reg[e] != want;
                            ++seen[mi][(size_t)row * rk[mi] + c + e];
                        }
                    }
                }
            }
        uint64_t not_once = 0, elements = 0, pieces_unused = 0;
        for (uint32_t m = 0; m < 4; ++m)
            for (uint8_t s : seen[m]) { ++elements; not_once += s != 1; }
        for (uint8_t p : piece_used) pieces_unused += p == 0;
        printf("{\"name\":\"%s\",\"pieces_per_head\":%u,\"bytes\":%zu,\"elements\":%llu,\"not_once\":%llu,\"mismatches\":%llu,\"pad_lanes\":%llu,"
               "\"pad_nonzero\":%llu,\"beyond_rank\":%llu,\"misaligned\":%llu,\"out_of_image\":%llu,\"twice\":%llu,\"pieces_unused\":%llu",
               name.c_str(), eng_l2_head_pieces(R), bytes, (unsigned long long)elements, (unsigned long long)not_once, (unsigned long long)mismatches,
               (unsigned long long)pad_lanes, (unsigned long long)pad_nonzero, (unsigned long long)beyond_rank, (unsigned long long)misaligned,
               (unsigned long long)out_of_image, (unsigned long long)twice, (unsigned long long)pieces_unused);
        printf(",\"unit_piece\":[");
        for (uint32_t u = 0; u <= 16; ++u) printf("%s%u", u ? "," : "", eng_l2_unit_piece(R, u));
        printf("]");
        if (dump) {
            printf(",\"image\":\"");
            for (uint8_t b : img) printf("%02x", b);
            printf("\"");
        }
        printf("}\n");
    }
    return 0;
}
