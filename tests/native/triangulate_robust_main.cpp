// triangulate_robust_main.cpp -- a stand-alone program around the host-emulated robust triangulation (tests/native/
// build_triangulate_robust_emu.py links it with triangulate.hip and emu_ctx.cpp under -fsanitize=address,undefined).  TEST INFRASTRUCTURE ONLY.
//
//   prog scene.bin result.bin   osfm_triangulate_bearings_robust over the scene, once with the file's draws and once with its seed
//   prog --unrank               reads "n id" lines, prints "i j" of unrank_pair (triangulate_robust.h, host side)
//   prog --draw                 reads "seed t k" lines, prints robust_draw as a hexadecimal float
//
// scene (little endian): int32 n_tracks, pad; int64 n_obs; double threshold, min_angle_deg, min_depth; int32 iterations, pad; uint64 seed;
//   int64 offsets[n_tracks + 1]; double centers[n_obs * 3]; double bearings[n_obs * 3]; double draws[n_tracks * 11]
// result: for each run (draws, then seed): double points[n_tracks * 3]; uint8 status[n_tracks]; uint8 mask[n_obs]; int32 n_inliers[n_tracks];
//   int32 tries[n_tracks]
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "osfm_mi355.h"
#include "triangulate_robust.h"

template <class T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "--unrank")) {
    long long n, id;
    while (scanf("%lld %lld", &n, &id) == 2) {
      int i = -1, j = -1;
      osfm_tri::unrank_pair((int64_t)id, (int)n, &i, &j);
      printf("%d %d\n", i, j);
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "--draw")) {
    unsigned long long seed;
    long long t;
    int k;
    while (scanf("%llu %lld %d", &seed, &t, &k) == 3) printf("%a\n", osfm_tri::robust_draw((uint64_t)seed, (int64_t)t, k));
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s scene.bin result.bin | --unrank | --draw\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[2], it[2];
  int64_t n_obs;
  double prm[3];
  uint64_t seed;
  if (fread(head, 4, 2, f) != 2 || fread(&n_obs, 8, 1, f) != 1 || fread(prm, 8, 3, f) != 3 || fread(it, 4, 2, f) != 2 || fread(&seed, 8, 1, f) != 1) return 2;
  const int n_tracks = head[0];
  std::vector<int64_t> offsets;
  std::vector<double> centers, bearings, draws;
  const bool ok = read_vec(f, offsets, (size_t)n_tracks + 1) && read_vec(f, centers, (size_t)n_obs * 3) && read_vec(f, bearings, (size_t)n_obs * 3) &&
                  read_vec(f, draws, (size_t)n_tracks * 11);
  fclose(f);
  if (!ok) return 2;
  osfm_triangulate_params p;
  osfm_triangulate_params_default(&p);
  p.threshold = prm[0];
  p.min_angle_deg = prm[1];
  p.min_depth = prm[2];
  p.refinement_iterations = it[0];
  osfm_ctx *ctx = nullptr;
  if (osfm_ctx_create(0, &ctx) != OSFM_OK) return 3;
  FILE *g = fopen(argv[2], "wb");
  if (!g) return 2;
  int rc = 0;
  for (int run = 0; run < 2 && rc == 0; run++) {
    std::vector<double> points((size_t)n_tracks * 3);
    std::vector<uint8_t> status((size_t)n_tracks), mask((size_t)n_obs);
    std::vector<int32_t> n_inliers((size_t)n_tracks), tries((size_t)n_tracks);
    double ms = 0.0;
    rc = osfm_triangulate_bearings_robust(ctx, centers.data(), bearings.data(), offsets.data(), n_tracks, &p, run == 0 ? draws.data() : nullptr, seed,
                                          points.data(), status.data(), mask.data(), n_inliers.data(), tries.data(), &ms);
    if (rc != OSFM_OK) {
      fprintf(stderr, "run %d: %d %s\n", run, rc, osfm_last_error());
      break;
    }
    fwrite(points.data(), 8, points.size(), g);
    fwrite(status.data(), 1, status.size(), g);
    fwrite(mask.data(), 1, mask.size(), g);
    fwrite(n_inliers.data(), 4, n_inliers.size(), g);
    fwrite(tries.data(), 4, tries.size(), g);
  }
  fclose(g);
  osfm_ctx_destroy(ctx);
  return rc == 0 ? 0 : 1;
}
