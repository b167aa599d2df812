// scan_host.hpp -- the tile of the exclusive prefix sums (scan.cuh), for the scratch layouts of the passes that scan: pure host code, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace egscan {

constexpr uint32_t SCAN_TILE = 1024;              // elements per block of the scan kernels
inline uint32_t scan_tiles(size_t n) { return (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE); }

}  // namespace egscan
