// The host-side helpers of csrc/vol_common.h on the CPU: both extents predicates, the NIfTI datatype table, the bounded-grid size, the 16-byte padding and the overlap
// test, printed for a fixed list of inputs so that a machine without a GPU can hold them to a Python restatement (tests/test_vol_common_host.py builds and runs it), and so
// that the host sanitizers can be put on them (-Xarch_host -fsanitize=undefined).  No device is touched: nothing is launched.
//     hipcc --offload-arch=gfx950 -O2 -std=c++17 -I <package>/csrc tools/vol_common_host_check.hip -o vol_common_host_check
// One line per input: the name of the helper, its arguments, its result.
#include "vol_common.h"

#include <cstdio>

int main() {
  const int M = 2147483647;
  const int dims[][3] = {{-1, 3, 2}, {3, -1, 2}, {3, 2, -1}, {0, 0, 0}, {5, 3, 0}, {1, 1, 1}, {512, 512, 301}, {2047, 1024, 1024}, {2048, 2048, 512}, {2048, 2048, 511},
                         {46340, 46340, 1}, {46341, 46341, 1}, {46341, 46341, 0}, {65536, 65536, 0}, {65536, 0, 65536}, {M, M, 0}, {0, M, M}, {M, 0, M}, {M, 1, 1}, {M, 1, 2},
                         {1, M, 1}, {1, 1, M}, {2, 1, M}, {M, M, 1}, {M, M, M}};
  for (const auto& d : dims) printf("dims %d %d %d %d %d\n", d[0], d[1], d[2], vol_dims_ok(d[0], d[1], d[2]) ? 1 : 0, vol_dims_ok_or_empty(d[0], d[1], d[2]) ? 1 : 0);
  const int dts[] = {0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304, -2};
  for (int dt : dts) printf("itemsize %d %d\n", dt, vol_itemsize(dt));
  const long long blocks[][3] = {{0, 8192, 256}, {-5, 8192, 256}, {1, 8192, 256}, {256, 8192, 256}, {257, 8192, 256}, {2097152, 8192, 256}, {2097153, 8192, 256},
                                 {2147483647LL, 8192, 256}, {4611686018427387904LL, 8192, 256}, {1000, 2048, 256}, {262144, 1024, 256}, {65536, 256, 256}, {1000, 8192, 64},
                                 {129, 8192, 128}, {1000, 1, 256}};
  for (const auto& b : blocks) printf("blocks %lld %lld %lld %u\n", b[0], b[1], b[2], vol_blocks(b[0], b[1], (int)b[2]));
  const unsigned long long pads[] = {0, 1, 15, 16, 17, 31, 32, 4096, 4097, 1ull << 40, (1ull << 40) + 1};
  for (unsigned long long b : pads) printf("pad16 %llu %llu\n", b, (unsigned long long)vol_pad16((size_t)b));
  const unsigned long long laps[][4] = {{4096, 16, 4112, 16}, {4096, 17, 4112, 16}, {4112, 16, 4096, 16}, {4112, 16, 4096, 17}, {4096, 64, 4100, 4}, {4100, 4, 4096, 64},
                                        {4096, 0, 4096, 16}, {4096, 16, 4096, 0}, {4096, 0, 4096, 0}, {4096, 1, 4096, 1}, {4097, 0, 4096, 16}};
  for (const auto& l : laps)
    printf("overlap %llu %llu %llu %llu %d\n", l[0], l[1], l[2], l[3],
           vol_overlap(reinterpret_cast<const void*>((uintptr_t)l[0]), (size_t)l[1], reinterpret_cast<const void*>((uintptr_t)l[2]), (size_t)l[3]) ? 1 : 0);
  const unsigned long long als[][2] = {{0, 16}, {4096, 16}, {4104, 16}, {4104, 8}, {4097, 1}, {4098, 4}};
  for (const auto& a : als) printf("aligned %llu %llu %d\n", a[0], a[1], vol_aligned(reinterpret_cast<const void*>((uintptr_t)a[0]), (size_t)a[1]) ? 1 : 0);
  return 0;
}
