// The decode engine's packed image of a layer's LoRA up-projections (w2, a2, g2, v2; F16 rows), free of HIP: the index arithmetic that
// the host packer (wrk_v7_engine_create), the head workgroups of v7_engine_kernel and the host test share.  DESIGN.md section 4.8.
// wrk_v7_engine.h includes it.
//
// A head workgroup multiplies 16 (matrix, 16-row block) units u = 4 mi + bi, matrix mi in the order w, a, g, v.  Lane L of the wave that
// owns a unit holds, in register n, columns [c, c + 8) with c = 8 (L & 3) + 32 n of row head * 64 + 16 bi + (L >> 2): four lanes cover 32
// columns of one row, a wave 16 rows.  In the matrices themselves such a register set is a 64-byte piece out of each of 16 rows.  The
// image stores it in LOAD order instead: a PIECE is the 1 KB that one wave-wide 16-byte load takes, lane L's 16 bytes at byte 16 L;
// piece n of a unit exists only if 32 n < rank (lanes with c >= rank hold zeros and are never multiplied); the pieces of a unit follow
// each other, the units of a head follow each other in the order of u, the heads in their own order.  The layout therefore does not
// depend on which wave owns a unit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef WRK_HD
#ifdef __HIPCC__
#define WRK_HD __host__ __device__
#else
#define WRK_HD
#endif
#endif

namespace wrk {

constexpr uint32_t ENG_L2_PIECE_BYTES = 1024;   // 64 lanes x 16 bytes
constexpr uint32_t ENG_L2_UNITS = 16;           // 4 matrices x 4 blocks of 16 rows of a head's 64
constexpr uint32_t ENG_L2_MAX_PIECES = 8;       // rank <= 256

// ranks of the four matrices, in unit order.  Four fields and selects, not an array: in a kernel an array that is indexed by a run-time
// value lives in scratch memory.
struct EngLora2Ranks { uint32_t w, a, g, v; };
WRK_HD constexpr uint32_t eng_l2_rank(const EngLora2Ranks& R, uint32_t m) { return m == 0u ? R.w : m == 1u ? R.a : m == 2u ? R.g : R.v; }
// pieces of one unit of a matrix of `rank` columns
WRK_HD constexpr uint32_t eng_l2_pieces(uint32_t rank) { return (rank + 31u) / 32u; }
// first piece of unit u (0 .. 16; 16 = pieces of a head) inside a head's run
WRK_HD constexpr uint32_t eng_l2_unit_piece(const EngLora2Ranks& R, uint32_t u) {
    const uint32_t m = u / 4u;
    const uint32_t whole = (m > 0u ? eng_l2_pieces(R.w) : 0u) + (m > 1u ? eng_l2_pieces(R.a) : 0u) + (m > 2u ? eng_l2_pieces(R.g) : 0u) +
                           (m > 3u ? eng_l2_pieces(R.v) : 0u);
    return 4u * whole + (u % 4u) * eng_l2_pieces(eng_l2_rank(R, m));
}
WRK_HD constexpr uint32_t eng_l2_head_pieces(const EngLora2Ranks& R) { return eng_l2_unit_piece(R, ENG_L2_UNITS); }
// piece (head, u, n) of a layer's image, n < eng_l2_pieces(eng_l2_rank(R, u / 4))
WRK_HD constexpr size_t eng_l2_piece(const EngLora2Ranks& R, uint32_t head, uint32_t u, uint32_t n) {
    return (size_t)head * eng_l2_head_pieces(R) + eng_l2_unit_piece(R, u) + n;
}
WRK_HD constexpr size_t eng_l2_layer_bytes(const EngLora2Ranks& R, uint32_t heads) {
    return (size_t)heads * eng_l2_head_pieces(R) * ENG_L2_PIECE_BYTES;
}
// what lane `lane` of piece (head, u, n) holds: 8 columns from `col` of row `row` of matrix u / 4
WRK_HD constexpr uint32_t eng_l2_src_row(uint32_t head, uint32_t u, uint32_t lane) { return head * 64u + 16u * (u % 4u) + lane / 4u; }
WRK_HD constexpr uint32_t eng_l2_src_col(uint32_t n, uint32_t lane) { return 8u * (lane % 4u) + 32u * n; }

// A column that no (piece, lane) holds is a product that K2 drops; one held twice is loaded for nothing; a unit that overlaps the next is
// a wrong weight.  So the arithmetic is proved at compile time, for every rank the engine accepts (multiples of 8 up to 256) in each of
// the four positions beside three other ranks: every 8-column group below the rank has exactly one (n, lane & 3), no piece starts at or
// beyond the rank, the last piece of a unit reaches the rank, and the units of a head are dense, in order, and add up to the head's run.
constexpr bool eng_l2_layout_ok() {
    for (uint32_t rank = 8; rank <= 256; rank += 8) {
        const uint32_t np = eng_l2_pieces(rank);
        if (np == 0 || np > ENG_L2_MAX_PIECES || 32u * (np - 1u) >= rank || 32u * np < rank) return false;
        for (uint32_t c = 0; c < rank; c += 8) {
            uint32_t owners = 0;
            for (uint32_t n = 0; n < np; ++n)
                for (uint32_t q = 0; q < 4; ++q) owners += eng_l2_src_col(n, q) == c ? 1u : 0u;
            if (owners != 1) return false;
        }
        for (uint32_t pos = 0; pos < 4; ++pos) {
            const EngLora2Ranks R{pos == 0 ? rank : 96u, pos == 1 ? rank : 40u, pos == 2 ? rank : 256u, pos == 3 ? rank : 8u};
            uint32_t next = 0;
            for (uint32_t u = 0; u < ENG_L2_UNITS; ++u) {
                if (eng_l2_unit_piece(R, u) != next) return false;
                next += eng_l2_pieces(eng_l2_rank(R, u / 4u));
            }
            if (eng_l2_head_pieces(R) != next || eng_l2_piece(R, 3, 0, 0) != 3u * next) return false;
        }
    }
    for (uint32_t lane = 0; lane < 64; ++lane)      // a piece is 16 rows x 4 lanes, rows in lane order
        if (eng_l2_src_row(2, 7, lane) != 2u * 64u + 48u + lane / 4u) return false;
    return true;
}
static_assert(eng_l2_layout_ok(), "LoRA-2 pack: a column without exactly one (piece, lane), or units that are not dense and in order");
// 1.5B: ranks 96 / 96 / 256 / 64 -> 3 + 3 + 8 + 2 pieces per block, 64 pieces = 64 KB per head
static_assert(eng_l2_head_pieces(EngLora2Ranks{96, 96, 256, 64}) == 64, "LoRA-2 pack: pieces of a 1.5B head");

// The host packer.  src[m]: matrix m (F16, `row_bytes[m]` apart, heads * 64 rows of eng_l2_rank(R, m) columns) or nullptr (layer 0 has no v2: its
// pieces stay zero, and K2 drops their dots).  dst: eng_l2_layer_bytes(R, heads) bytes.
inline void eng_l2_pack_layer(const EngLora2Ranks& R, uint32_t heads, const uint8_t* const (&src)[4], const size_t (&row_bytes)[4], uint8_t* dst) {
    for (uint32_t head = 0; head < heads; ++head)
        for (uint32_t u = 0; u < ENG_L2_UNITS; ++u) {
            const uint32_t m = u / 4u, rank = eng_l2_rank(R, m);
            for (uint32_t n = 0; n < eng_l2_pieces(rank); ++n) {
                uint8_t* piece = dst + eng_l2_piece(R, head, u, n) * ENG_L2_PIECE_BYTES;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t c = eng_l2_src_col(n, lane);
                    for (uint32_t b = 0; b < 16; ++b)
                        piece[16u * lane + b] = (src[m] && c < rank) ? src[m][(size_t)eng_l2_src_row(head, u, lane) * row_bytes[m] + 2u * c + b] : 0;
                }
            }
        }
}

}  // namespace wrk
