// Host-side helpers shared by the C-ABI translation units: error reporting and the global zero page.
#pragma once
#include <hip/hip_runtime.h>

int y5_fail(int code, const char* msg);           // records msg for y5_last_error(), returns code
int y5_check_launch(const char* what);            // hipGetLastError() -> status
const void* y5_zero_page();                       // device buffer of zeros (per device), nullptr on failure
int y5_num_cu();                                  // CUs persistent grids are sized for: the device's count, capped by y5_set_cu_budget()

// workgroups of a persistent grid: max_blocks when the caller caps it, else as many as stay resident (CUs x occupancy of `kern`)
inline long long y5_resident_slots(const void* kern, int threads, size_t lds, int max_blocks) {
  if (max_blocks > 0) return max_blocks;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, lds) != hipSuccess || occ < 1) occ = 1;
  return (long long)y5_num_cu() * occ;
}
