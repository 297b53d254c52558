// Prints k_rdx's hand-off place map (fmcw_radar_processing_amd/csrc/xcd_place.h) for tests/test_xcd_place.py:
// one line "j r w place" per team step j = 0 .. steps - 1, reader member r and writer member w, then the
// place and row pitch.  The checks themselves are in the Python test.
//
//   g++ -std=c++17 tests/native/xcd_place.cpp -o xcd_place && ./xcd_place 6
#include <cstdio>
#include <cstdlib>

#include "../../fmcw_radar_processing_amd/csrc/xcd_place.h"

int main(int argc, char** argv) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 6;
  for (int j = 0; j < steps; ++j)
    for (int r = 0; r < 32; ++r)
      for (int w = 0; w < 32; ++w) std::printf("%d %d %d %d\n", j, r, w, fmcw::xcd_place(j, r, w));
  std::printf("pitch %d %d\n", fmcw::XCD_PLACE_BYTES, fmcw::XCD_ROW_BYTES);
  return 0;
}
