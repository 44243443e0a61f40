// The per-voxel arithmetic of csrc/kernels_vessel.hip on the CPU: the kernel file's own __host__ __device__ functions (vs_eigenvalues, vs_measure) behind a host copy of
// its brick walk and staging, so that a machine without a GPU can hold the kernel's arithmetic to tests/vessel_oracle.py bit for bit (tests/test_vessel_host.py builds and
// runs it), and so that the host sanitizers can be put on it (-Xarch_host -fsanitize=address,undefined).  No device is touched: nothing is launched.
//     hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -I <package>/csrc tools/vessel_host_check.hip -o vessel_host_check
//     vessel_host_check X Y Z in.bin bright out.bin
// in.bin: X Y Z float32 (Fortran order), then nine float64: the six factors and the three denominators.  out.bin: l1 | l2 | l3 | response, four float32 volumes.
#include "kernels_vessel.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: %s X Y Z in.bin bright out.bin\n", argv[0]); return 2; }
  const int X = atoi(argv[1]), Y = atoi(argv[2]), Z = atoi(argv[3]);
  if (X <= 0 || Y <= 0 || Z <= 0 || (long long)X * Y * Z >= 0x80000000LL) { fprintf(stderr, "bad extents\n"); return 2; }
  const long long N = (long long)X * Y * Z;
  std::vector<float> L(N), out(4 * N), s(S);
  double k[9];
  FILE* f = fopen(argv[4], "rb");
  if (!f || fread(L.data(), 4, N, f) != (size_t)N || fread(k, 8, 9, f) != 9) { fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
  fclose(f);
  const vs_params P{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], atoi(argv[5]) != 0 ? 1 : 0, 0};
  float qnan;
  memcpy(&qnan, &QNAN_BITS, 4);
  const int nbx = (X + BX - 1) / BX, nby = (Y + BY - 1) / BY, nbz = (Z + BZ - 1) / BZ;
  for (int bz = 0; bz < nbz; ++bz)
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) {
        const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
        for (int i = 0; i < S; ++i) {                                 // the brick and its halo, the edge voxel repeating: as the kernel stages it
          const int sx = i % SX, t = i / SX, sy = t % SY, sz = t / SY;
          const long long px = std::min(std::max((long long)x0 + sx - 1, 0LL), (long long)X - 1), py = std::min(std::max((long long)y0 + sy - 1, 0LL), (long long)Y - 1),
                          pz = std::min(std::max((long long)z0 + sz - 1, 0LL), (long long)Z - 1);
          s[i] = L[px + X * (py + Y * pz)];
        }
        for (int l = 0; l < BRICK; ++l) {
          const int lx = l & (BX - 1), ly = (l >> 5) & (BY - 1), lz = l >> 8, gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
          if (gx >= X || gy >= Y || gz >= Z) continue;
          const long long v = gx + (long long)X * (gy + (long long)Y * gz);
          double l1, l2, l3;
          const bool finite = vs_eigenvalues(s.data(), (lx + 1) + SX * ((ly + 1) + SY * (lz + 1)), P, l1, l2, l3);
          out[v] = finite ? (float)l1 : qnan; out[N + v] = finite ? (float)l2 : qnan; out[2 * N + v] = finite ? (float)l3 : qnan;
          out[3 * N + v] = finite ? vs_measure(l1, l2, l3, P) : 0.0f;
        }
      }
  f = fopen(argv[6], "wb");
  if (!f || fwrite(out.data(), 4, 4 * N, f) != (size_t)(4 * N)) { fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
  fclose(f);
  return 0;
}
