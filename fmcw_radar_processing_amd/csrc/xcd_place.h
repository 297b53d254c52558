// Where a chunk of the range cube lives in k_rdx's hand-off slot (kernels_xcd.hip).  No HIP types:
// tests/native/xcd_place.cpp prints the map on the host and tests/test_xcd_place.py checks it.
//
// The slot (one per XCD, 2 MiB) is 1024 places of 2 KiB.  Chunk (r, w) of a frame -- the 8 chirps
// 8 w .. 8 w + 7 that writer member w produces for reader member r, 32 bins of group r each, one 256-byte
// row per chirp (wave v's chirp 8 w + v at byte 256 v; a c32h row uses its first 128 bytes) -- lives at
// place xcd_place(j, r, w) in team step j: [group][chirp][32] on even steps, its transpose over (r, w)
// on odd ones.  xcd_place(j + 1, a, b) == xcd_place(j, b, a): the rows wave v of member k stores for
// frame j + 1 (chunks (g, k), row v) are exactly the rows it loaded of frame j (chunks (k, g), row v),
// and no other wave reads them.  A wave therefore only overwrites bytes it has itself just read, and one
// slot needs no write-after-read protection between members: each place goes back and forth between one
// fixed pair of members (A writes, B reads, B writes, A reads).
#pragma once

namespace fmcw {

constexpr int XCD_PLACE_BYTES = 2048, XCD_ROW_BYTES = 256;
// (constexpr: usable in host and device code alike)
constexpr int xcd_place(int j, int r, int w) { return (j & 1) ? 32 * w + r : 32 * r + w; }

}  // namespace fmcw
