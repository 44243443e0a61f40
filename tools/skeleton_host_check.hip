// The thinning of csrc/kernels_skeleton.hip on the CPU: the kernel file's own __host__ __device__ functions (sk_simple, sk_candidates_word, sk_recheck_word,
// sk_subfield_bits) behind a host copy of its launch sequence, so that a machine without a GPU can hold the kernel's predicate and its per-word work to
// tests/skeleton_oracle.py bit for bit (tests/test_skeleton_host.py builds and runs it), and so that the host sanitizers can be put on it
// (-Xarch_host -fsanitize=address,undefined).  No device is touched: nothing is launched.
//     hipcc --offload-arch=gfx950 -O2 -std=c++17 -I <package>/csrc tools/skeleton_host_check.hip -o skeleton_host_check
//     skeleton_host_check count                                        prints the number of simple neighbourhoods among all 2^26
//     skeleton_host_check thin X Y Z in.bin endpoints max_iterations out.bin
// in.bin: X Y Z bytes (Fortran order).  max_iterations < 0: until an iteration clears nothing.  out.bin: X Y Z bytes 0 / 1.  Prints "iterations n" and "removed r0 r1 ...".
#include "kernels_skeleton.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int count_simple() {
  long long n = 0;
  for (uint32_t c = 0; c < (1u << 26); ++c) n += sk_simple(c) ? 1 : 0;
  printf("%lld\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "count")) return count_simple();
  if (argc != 9 || strcmp(argv[1], "thin")) { fprintf(stderr, "usage: %s count | thin X Y Z in.bin endpoints max_iterations out.bin\n", argv[0]); return 2; }
  const int X = atoi(argv[2]), Y = atoi(argv[3]), Z = atoi(argv[4]), endpoints = atoi(argv[6]) != 0;
  const long long max_it = atoll(argv[7]);
  if (X <= 0 || Y <= 0 || Z <= 0 || !vol_dims_ok(X, Y, Z)) { fprintf(stderr, "bad extents\n"); return 2; }
  const vol_bits d = vol_bits_make(X, Y, Z);
  std::vector<uint8_t> vol(d.N);
  FILE* f = fopen(argv[5], "rb");
  if (!f || fread(vol.data(), 1, d.N, f) != (size_t)d.N) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
  fclose(f);
  std::vector<u64> P(d.words, 0ull), Q(d.words, 0ull), next(d.words);
  for (long long w = 0; w < d.words; ++w) {                            // sk_pack_kernel
    const long long row = w / d.WX;
    const int x0 = (int)(w - row * d.WX) * 64;
    for (int b = 0; b < 64 && x0 + b < X; ++b)
      if (vol[row * X + x0 + b]) P[w] |= 1ull << b;
  }
  std::vector<long long> removed;
  while (max_it < 0 || (long long)removed.size() < max_it) {
    long long cleared = 0;
    for (int dir = 0; dir < 6; ++dir) {
      for (long long w = 0; w < d.words; ++w) Q[w] = sk_candidates_word(P.data(), d, w, dir, endpoints ? 2 : 1);          // sk_candidates_kernel
      for (int k = 0; k < 8; ++k) {                                  // sk_recheck_kernel: every lane reads the image as the launch found it -- the strictest reading of "at once"
        next = P;
        for (long long w = 0; w < d.words; ++w) {
          const long long row = w / d.WX;
          const int z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
          const u64 cand = Q[w] & sk_subfield_bits(k, y, z);
          if (!cand) continue;
          const u64 clear = sk_recheck_word(P.data(), d, w, cand);
          next[w] &= ~clear;
          cleared += sk_popc64(clear);
        }
        P.swap(next);
      }
    }
    removed.push_back(cleared);
    if (!cleared) break;
  }
  for (long long w = 0; w < d.words; ++w) {                            // sk_unpack_kernel
    const long long row = w / d.WX;
    const int x0 = (int)(w - row * d.WX) * 64;
    for (int b = 0; b < 64 && x0 + b < X; ++b) vol[row * X + x0 + b] = (uint8_t)((P[w] >> b) & 1ull);
  }
  f = fopen(argv[8], "wb");
  if (!f || fwrite(vol.data(), 1, d.N, f) != (size_t)d.N) { fprintf(stderr, "cannot write %s\n", argv[8]); return 2; }
  fclose(f);
  printf("iterations %zu\nremoved", removed.size());
  for (long long r : removed) printf(" %lld", r);
  printf("\n");
  return 0;
}
