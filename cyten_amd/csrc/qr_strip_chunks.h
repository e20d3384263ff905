// Row-split strips of the blocked QR (blocked_qr.hip: strip_w1_kernel + strip_apply_kernel): the arithmetic that cuts a
// strip of mr rows into chunks.  It decides how many 32 x 32 partials a panel step writes into a workspace that was sized
// earlier from strip_slot_bound, so the two must agree: tests/qr_strip_chunks.cpp walks them on the host.  No HIP in here;
// the switches (CYB_QR_CHUNK_ROWS, CYB_QR_CHUNK_MIN) are read in blocked_qr.hip and arrive as `mode` and `ch_min`.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace cyb {

// The chunk size is chosen PER PANEL STEP so that the chunk workgroups of the step fit the chip once (one workgroup per CU:
// the kernels use the whole register file): a single large matrix has ~45 strips per step and is cut into chunks of 384
// rows, a list whose strips fill the chip anyway is not cut at all (two launches of two rounds each measured SLOWER than the
// one-launch strip kernel there: chi=4096 list 26.3 -> 28.9 ms with a fixed 384, single 1442^2 block 20.9 -> 17.4 ms).
constexpr int kChunkRowsMin = 192;
constexpr int kChunkRowsChoices[] = {192, 256, 384, 512, 768, 1024, 1536};

// mode: -1 = adaptive, 0 = never split, n = fixed chunk rows (multiple of 16)
// upper bound of strip_chunks(rows, ch) for every ch the mode can choose
inline int strip_slot_bound(int64_t rows, int mode)
{
    if (mode == 0) return 1;
    const int ch = mode > 0 ? std::min(mode, kChunkRowsMin) : kChunkRowsMin; // (the bound for every choice)
    return (int)std::max<int64_t>(1, (rows + ch - 1) / ch);
}
// rows per chunk of a strip of mr rows cut into chunks of at most ch rows: even shares, multiples of 16 rows (ch == 0: one chunk)
inline int strip_chunk_share(int mr, int ch)
{
    if (ch <= 0 || mr <= ch) return std::max(mr, 1);
    const int ns = (mr + ch - 1) / ch;
    return ((mr + ns - 1) / ns + 15) / 16 * 16;
}
inline int strip_chunks(int mr, int ch)
{
    const int share = strip_chunk_share(mr, ch);
    return std::max(1, (mr + share - 1) / share);
}
// chunk sl < strip_chunks(mr, ch) of the strip: its first row and its rows
struct StripChunk {
    int row0, rows;
};
inline StripChunk strip_chunk(int mr, int ch, int sl)
{
    const int share = strip_chunk_share(mr, ch), r0 = sl * share;
    return StripChunk{r0, std::min(share, mr - r0)};
}
// chunk rows of a panel step whose strips are (rows, count) pairs; 0: no split (the one-launch strip kernel)
inline int choose_chunk_rows(const std::vector<std::pair<int, int>>& strips, int n_cu, int mode, int ch_min)
{
    if (mode == 0) return 0;
    if (mode > 0) return mode;
    int64_t n_strips = 0;
    for (const auto& s : strips) n_strips += s.second;
    if (n_strips == 0 || n_strips * 4 > (int64_t)n_cu * 3) return 0; // the strips fill three quarters of the chip: leave them whole
    for (int ch : kChunkRowsChoices) {
        if (ch < ch_min) continue;
        int64_t tot = 0;
        bool any = false;
        for (const auto& s : strips) {
            const int c = strip_chunks(s.first, ch);
            tot += (int64_t)c * s.second;
            any = any || c > 1;
        }
        if (tot <= n_cu) return any ? ch : 0;
    }
    return 0;
}

} // namespace cyb
