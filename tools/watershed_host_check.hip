// The sweeps of csrc/kernels_watershed.hip on the CPU: the kernel file's own __host__ __device__ functions (ws_relax_height / _label / _sum, ws_seed, ws_brick_active)
// behind a host copy of its launch sequence -- bricks of 32 x 8 x 8 staged with a frozen halo of 1, relaxed to their own fixed point, written to the other key buffer, the
// per-brick flags ping-ponged, the skip rule applied -- so that a machine without a GPU can hold the relaxation, the ping-pong and the skip argument to
// tests/watershed_oracle.py bit for bit (tests/test_watershed_host.py builds and runs it), and so that the host sanitizers can be put on it
// (-Xarch_host -fsanitize=address,undefined).  No device is touched: nothing is launched.
//     hipcc --offload-arch=gfx950 -O2 -std=c++17 -I <package>/csrc tools/watershed_host_check.hip -o watershed_host_check
//     watershed_host_check X Y Z connectivity rule skip cost.bin markers.bin mask.bin out.bin
// rule: max | sum.  cost.bin: X Y Z uint32, markers.bin: X Y Z int32, mask.bin: X Y Z bytes (Fortran order).  out.bin: labels int32 [N], then for max height uint32 [N] and
// steps uint32 [N], for sum distance uint64 [N].  Prints, per phase, "changed c0 c1 ..." (to the first sweep that changed nothing) and at last "counts r u o i".
#include "kernels_watershed.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <typename T>
static bool read_all(const char* path, std::vector<T>& v) {
  FILE* f = fopen(path, "rb");
  const bool ok = f && fread(v.data(), sizeof(T), v.size(), f) == v.size();
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "cannot read %s\n", path);
  return ok;
}

struct volume {
  ws_dims d;
  std::vector<uint32_t> cost, H;
  std::vector<int32_t> markers;
  std::vector<uint8_t> mask, bmask, F[2];
  std::vector<u64> K[2];
};

static long long brick_of(const ws_dims& d, int x, int y, int z) { return (x / WS_BX) + (long long)d.NBX * ((y / WS_BY) + (long long)d.NBY * (z / WS_BZ)); }

// ws_seed_kernel
static void seed(volume& v, int phase, int done) {
  const ws_dims& d = v.d;
  if (phase == WS_LABEL)
    for (long long f = 0; f < d.N; ++f) { const u64 h = v.K[done & 1][f]; v.H[f] = h == WS_UNREACHED ? WS_H_UNREACHED : (uint32_t)h; }
  std::fill(v.bmask.begin(), v.bmask.end(), 0);
  std::fill(v.F[0].begin(), v.F[0].end(), 1);
  for (long long f = 0; f < d.N; ++f) {
    const bool inmask = v.mask[f] != 0;
    v.K[0][f] = v.K[1][f] = ws_seed(phase, inmask, v.markers[f], v.cost[f]);
    if (inmask) { const long long row = f / d.X; v.bmask[brick_of(d, (int)(f - row * d.X), (int)(row % d.Y), (int)(row / d.Y))] = 1; }
  }
}

// ws_sweep_kernel: sweep s of a phase -> the voxels it lowered
static long long sweep(volume& v, int s, int phase, int conn, int skip) {
  const ws_dims& d = v.d;
  const std::vector<u64>& R = v.K[s & 1];
  std::vector<u64>& W = v.K[(s + 1) & 1];
  const std::vector<uint8_t>& FR = v.F[s & 1];
  std::vector<uint8_t>& FW = v.F[(s + 1) & 1];
  std::vector<u64> k(WS_HALO), nw(WS_HALO);
  std::vector<uint32_t> h(WS_HALO);
  long long total = 0;
  for (long long b = 0; b < d.nb; ++b) {
    if (!v.bmask[b] || (skip && !ws_brick_active(FR.data(), d, b))) { FW[b] = 0; continue; }
    const long long brow = b / d.NBX;
    const int x0 = (int)(b - brow * d.NBX) * WS_BX, z0 = (int)(brow / d.NBY) * WS_BZ, y0 = (int)(brow % d.NBY) * WS_BY;
    for (int i = 0; i < WS_HALO; ++i) {
      const int hx = i % WS_HX, hr = i / WS_HX, hy = hr % WS_HY, hz = hr / WS_HY, x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
      const bool in = x >= 0 && x < d.X && y >= 0 && y < d.Y && z >= 0 && z < d.Z;
      const long long f = x + (long long)d.X * (y + (long long)d.Y * z);
      k[i] = in ? R[f] : WS_UNREACHED;
      h[i] = in ? v.H[f] : WS_H_UNREACHED;
    }
    for (bool any = true; any;) {                                     // a pass: every voxel from the state the pass found, as the kernel's two barriers make it
      any = false;
      nw = k;
      for (int lz = 0; lz < WS_BZ; ++lz)
        for (int ly = 0; ly < WS_BY; ++ly)
          for (int lx = 0; lx < WS_BX; ++lx) {
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= d.X || y >= d.Y || z >= d.Z) continue;
            const long long f = x + (long long)d.X * (y + (long long)d.Y * z);
            if (!v.mask[f] || ws_marker_ok(v.markers[f])) continue;
            const int c = (lx + 1) + WS_HX * ((ly + 1) + WS_HY * (lz + 1));
            nw[c] = ws_relax(phase, k.data(), h.data(), c, WS_HX, WS_HX * WS_HY, conn, v.cost[f], k[c]);
            any = any || nw[c] != k[c];
          }
      k.swap(nw);
    }
    long long cnt = 0;
    for (int lz = 0; lz < WS_BZ; ++lz)
      for (int ly = 0; ly < WS_BY; ++ly)
        for (int lx = 0; lx < WS_BX; ++lx) {
          const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
          if (x >= d.X || y >= d.Y || z >= d.Z) continue;
          const long long f = x + (long long)d.X * (y + (long long)d.Y * z);
          const u64 val = k[(lx + 1) + WS_HX * ((ly + 1) + WS_HY * (lz + 1))];
          cnt += val != R[f];
          W[f] = val;
        }
    FW[b] = cnt != 0;
    total += cnt;
  }
  return total;
}

// _begin, then _sweeps until one changes nothing -> the sweeps run
static int run_phase(volume& v, int phase, int conn, int skip, int done) {
  seed(v, phase, done);
  printf("changed");
  int s = 0;
  for (;;) {
    const long long c = sweep(v, s++, phase, conn, skip);
    printf(" %lld", c);
    if (!c) break;
  }
  printf("\n");
  return s;
}

int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: %s X Y Z connectivity max|sum skip cost.bin markers.bin mask.bin out.bin\n", argv[0]); return 2; }
  const int X = atoi(argv[1]), Y = atoi(argv[2]), Z = atoi(argv[3]), conn = atoi(argv[4]), skip = atoi(argv[6]) != 0;
  const bool sum = !strcmp(argv[5], "sum");
  if (X <= 0 || Y <= 0 || Z <= 0 || !vol_dims_ok(X, Y, Z) || conn < 1 || conn > 3 || (!sum && strcmp(argv[5], "max"))) { fprintf(stderr, "bad arguments\n"); return 2; }
  volume v;
  v.d = ws_dims_make(X, Y, Z);
  const ws_dims& d = v.d;
  v.cost.resize(d.N); v.H.assign(d.N, WS_H_UNREACHED); v.markers.resize(d.N); v.mask.resize(d.N);
  v.bmask.resize(d.nb); v.F[0].resize(d.nb); v.F[1].resize(d.nb); v.K[0].resize(d.N); v.K[1].resize(d.N);
  if (!read_all(argv[7], v.cost) || !read_all(argv[8], v.markers) || !read_all(argv[9], v.mask)) return 2;
  int done;
  if (sum) done = run_phase(v, WS_SUM, conn, skip, 0);
  else done = run_phase(v, WS_LABEL, conn, skip, run_phase(v, WS_HEIGHT, conn, skip, 0));
  const std::vector<u64>& K = v.K[done & 1];
  if (v.K[0] != v.K[1]) { fprintf(stderr, "the two key buffers differ after a sweep that changed nothing\n"); return 1; }
  // ws_unpack_kernel
  std::vector<int32_t> labels(d.N);
  std::vector<uint32_t> steps(d.N);
  std::vector<u64> dist(d.N);
  long long reached = 0, unreached = 0, overflowed = 0, invalid = 0;
  for (long long f = 0; f < d.N; ++f) {
    const u64 k = K[f];
    const bool got = k != WS_UNREACHED;
    labels[f] = !got ? 0 : sum ? (int32_t)(k & 0xFFFFFFull) : (int32_t)(uint32_t)k;
    steps[f] = got ? (uint32_t)(k >> 32) : WS_H_UNREACHED;
    dist[f] = k >> 24;
    if (v.markers[f] != 0 && !ws_marker_ok(v.markers[f])) ++invalid;
    if (got) { ++reached; continue; }
    if (!v.mask[f]) continue;
    ++unreached;
    if (!sum) continue;
    const long long row = f / d.X;
    const int x = (int)(f - row * d.X), z = (int)(row / d.Y), y = (int)(row % d.Y);
    bool beside = false;
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int n = (dx != 0) + (dy != 0) + (dz != 0), xx = x + dx, yy = y + dy, zz = z + dz;
          if (n == 0 || n > conn || xx < 0 || xx >= X || yy < 0 || yy >= Y || zz < 0 || zz >= Z) continue;
          if (K[xx + (long long)X * (yy + (long long)Y * zz)] != WS_UNREACHED) beside = true;
        }
    overflowed += beside;
  }
  FILE* f = fopen(argv[10], "wb");
  bool ok = f && fwrite(labels.data(), 4, d.N, f) == (size_t)d.N;
  if (ok && sum) ok = fwrite(dist.data(), 8, d.N, f) == (size_t)d.N;
  if (ok && !sum) ok = fwrite(v.H.data(), 4, d.N, f) == (size_t)d.N && fwrite(steps.data(), 4, d.N, f) == (size_t)d.N;
  if (f) fclose(f);
  if (!ok) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
  printf("counts %lld %lld %lld %lld\n", reached, unreached, overflowed, invalid);
  return 0;
}
