// Host check of csrc/qr_strip_chunks.h (built by test_qr_strip_chunks_host.py with ASan and UBSan).  A panel step of the
// blocked QR writes one 32 x 32 partial per chunk into a workspace that was sized earlier from strip_slot_bound: the walk
// below requires that the chunks of every strip cover its rows exactly once and never outnumber that bound, and the
// literals pin choose_chunk_rows to the rule the strips have always been cut by.
#include "qr_strip_chunks.h"

#include <cstdio>

using namespace cyb;

static int failures = 0;

#define EXPECT(cond, ...)                                                                                                                  \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures <= 20) std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__), std::printf(__VA_ARGS__), std::printf("\n");        \
        }                                                                                                                                  \
    } while (0)

// a strip of mr rows cut at ch under `mode` (-1: adaptive, 0: never split, n: fixed chunk rows)
static void check_strip(int mr, int ch, int mode)
{
    const int nch = strip_chunks(mr, ch);
    EXPECT(nch >= 1, "mr %d ch %d: %d chunks", mr, ch, nch);
    EXPECT(nch <= strip_slot_bound(mr, mode), "mr %d ch %d mode %d: %d chunks, %d slots", mr, ch, mode, nch, strip_slot_bound(mr, mode));
    int next = 0;
    for (int sl = 0; sl < nch; ++sl) {
        const StripChunk c = strip_chunk(mr, ch, sl);
        EXPECT(c.row0 == next, "mr %d ch %d: chunk %d starts at row %d, expected %d", mr, ch, sl, c.row0, next);
        EXPECT(c.row0 % 16 == 0, "mr %d ch %d: chunk %d starts at row %d, no multiple of 16", mr, ch, sl, c.row0);
        EXPECT(c.rows >= 1, "mr %d ch %d: chunk %d has %d rows", mr, ch, sl, c.rows);
        EXPECT(ch <= 0 || c.rows <= ch || nch == 1, "mr %d ch %d: chunk %d has %d rows", mr, ch, sl, c.rows);
        next = c.row0 + c.rows;
    }
    EXPECT(next == mr, "mr %d ch %d: covered up to row %d", mr, ch, next);
}

static void check_rows(int mr)
{
    check_strip(mr, 0, 0);
    check_strip(mr, 0, -1); // (the adaptive rule may leave a step whole)
    for (int ch : kChunkRowsChoices) check_strip(mr, ch, -1);
    for (int ch : {16, 64, 208}) check_strip(mr, ch, ch);
}

typedef std::vector<std::pair<int, int>> Strips; // (rows, count)

int main()
{
    for (int mr : {1, 15, 16, 17, 191, 192, 193, 383, 384, 385, 1536, 1537, 1664, 3071, 3072, 3073}) check_rows(mr);
    for (int mr = 1; mr <= 4096; ++mr) check_rows(mr);

    // shares and counts by hand: 1442 rows at 384 -> 4 chunks of ceil(1442 / 4) = 361 rounded up to 368 rows
    EXPECT(strip_chunk_share(1442, 384) == 368 && strip_chunks(1442, 384) == 4, "1442 rows at 384: share %d, %d chunks", strip_chunk_share(1442, 384), strip_chunks(1442, 384));
    EXPECT(strip_chunks(1442, 192) == 8 && strip_chunks(1442, 256) == 6, "1442 rows at 192 / 256: %d / %d chunks", strip_chunks(1442, 192), strip_chunks(1442, 256));
    EXPECT(strip_chunk(1442, 384, 3).row0 == 1104 && strip_chunk(1442, 384, 3).rows == 338, "1442 rows at 384: last chunk");
    EXPECT(strip_slot_bound(1442, -1) == 8 && strip_slot_bound(1442, 0) == 1 && strip_slot_bound(1442, 64) == 23 && strip_slot_bound(1442, 208) == 8, "slot bounds of 1442 rows");

    // choose_chunk_rows at 256 CUs, adaptive, smallest choice 192
    const int n_cu = 256;
    // one 1442-row matrix, 45 strips: 8 and 6 chunks per strip (360, 270 workgroups) do not fit, 4 (180) do
    EXPECT(choose_chunk_rows(Strips{{1442, 45}}, n_cu, -1, kChunkRowsMin) == 384, "single 1442-row matrix: %d", choose_chunk_rows(Strips{{1442, 45}}, n_cu, -1, kChunkRowsMin));
    // 193 strips are more than three quarters of 256 CUs: left whole (192 are not: 1 chunk each at 1536 is no cut, 2 each at 1024 is 384 > 256 ...)
    EXPECT(choose_chunk_rows(Strips{{1442, 193}}, n_cu, -1, kChunkRowsMin) == 0, "strips fill the chip: %d", choose_chunk_rows(Strips{{1442, 193}}, n_cu, -1, kChunkRowsMin));
    EXPECT(choose_chunk_rows(Strips{{1442, 100}, {721, 93}}, n_cu, -1, kChunkRowsMin) == 0, "strips of two matrices fill the chip");
    EXPECT(choose_chunk_rows(Strips{}, n_cu, -1, kChunkRowsMin) == 0, "empty list");
    EXPECT(choose_chunk_rows(Strips{{1442, 0}}, n_cu, -1, kChunkRowsMin) == 0, "list of no strips");
    // 150 strips of 3200 rows: even at 1536 every strip is 3 chunks, 450 workgroups
    EXPECT(choose_chunk_rows(Strips{{3200, 150}}, n_cu, -1, kChunkRowsMin) == 0, "no choice fits: %d", choose_chunk_rows(Strips{{3200, 150}}, n_cu, -1, kChunkRowsMin));
    // 100 strips of 150 rows fit at 192, where none of them is cut
    EXPECT(choose_chunk_rows(Strips{{150, 100}}, n_cu, -1, kChunkRowsMin) == 0, "smallest fitting choice cuts nothing: %d", choose_chunk_rows(Strips{{150, 100}}, n_cu, -1, kChunkRowsMin));
    // ... and the same with one strip that the choice does cut: 100 + 2 workgroups at 192
    EXPECT(choose_chunk_rows(Strips{{150, 100}, {200, 1}}, n_cu, -1, kChunkRowsMin) == 192, "one strip is cut at 192");
    // a larger minimum skips the smaller choices; the fixed modes do not look at the list
    EXPECT(choose_chunk_rows(Strips{{1442, 45}}, n_cu, -1, 512) == 512, "minimum 512: %d", choose_chunk_rows(Strips{{1442, 45}}, n_cu, -1, 512));
    EXPECT(choose_chunk_rows(Strips{{1442, 193}}, n_cu, 208, kChunkRowsMin) == 208 && choose_chunk_rows(Strips{{1442, 45}}, n_cu, 0, kChunkRowsMin) == 0, "fixed modes");

    if (failures) {
        std::printf("%d mismatches\n", failures);
        return 1;
    }
    std::printf("no mismatch\n");
    return 0;
}
