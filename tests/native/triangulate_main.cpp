// triangulate_main.cpp -- a stand-alone program around the host-emulated triangulation (tests/native/build_triangulate_emu.py links it with
// triangulate.hip and emu_ctx.cpp under -fsanitize=address,undefined): reads a scene from a file, runs both entry points and writes the
// results.  TEST INFRASTRUCTURE ONLY.
//
// file (little endian): int32 n_tracks, n_shots, n_cams, pad; int64 n_obs; double threshold, min_angle_deg, min_depth; int32 iterations, pad;
//   int64 offsets[n_tracks + 1]; double shot_pose[n_shots * 12]; int32 shot_camera[n_shots]; int32 cam_model[n_cams];
//   double cam_params[n_cams * 16]; int32 obs_shot[n_obs]; double obs_xy[n_obs * 2]; double centers[n_obs * 3]; double bearings[n_obs * 3]
// output: for each entry point (tracks, then bearings): double points[n_tracks * 3]; uint8 status[n_tracks]; int32 iterations[n_tracks]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "osfm_mi355.h"

template <class T>
static bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s scene.bin result.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[4];
  int64_t n_obs;
  double prm[3];
  int32_t it[2];
  if (fread(head, 4, 4, f) != 4 || fread(&n_obs, 8, 1, f) != 1 || fread(prm, 8, 3, f) != 3 || fread(it, 4, 2, f) != 2) return 2;
  const int n_tracks = head[0], n_shots = head[1], n_cams = head[2];
  std::vector<int64_t> offsets;
  std::vector<double> shot_pose, cam_params, obs_xy, centers, bearings;
  std::vector<int32_t> shot_camera, cam_model, obs_shot;
  const bool ok = read_vec(f, offsets, (size_t)n_tracks + 1) && read_vec(f, shot_pose, (size_t)n_shots * 12) && read_vec(f, shot_camera, (size_t)n_shots) &&
                  read_vec(f, cam_model, (size_t)n_cams) && read_vec(f, cam_params, (size_t)n_cams * 16) && read_vec(f, obs_shot, (size_t)n_obs) &&
                  read_vec(f, obs_xy, (size_t)n_obs * 2) && read_vec(f, centers, (size_t)n_obs * 3) && read_vec(f, bearings, (size_t)n_obs * 3);
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
  for (int entry = 0; entry < 2 && rc == 0; entry++) {
    std::vector<double> points((size_t)n_tracks * 3);
    std::vector<uint8_t> status((size_t)n_tracks);
    std::vector<int32_t> iterations((size_t)n_tracks);
    double ms = 0.0;
    rc = entry == 0 ? osfm_triangulate_tracks(ctx, shot_pose.data(), shot_camera.data(), n_shots, cam_model.data(), cam_params.data(), n_cams,
                                              obs_shot.data(), obs_xy.data(), offsets.data(), n_tracks, &p, points.data(), status.data(),
                                              iterations.data(), &ms)
                    : osfm_triangulate_bearings(ctx, centers.data(), bearings.data(), offsets.data(), n_tracks, &p, points.data(), status.data(),
                                                iterations.data(), &ms);
    if (rc != OSFM_OK) {
      fprintf(stderr, "entry %d: %d %s\n", entry, rc, osfm_last_error());
      break;
    }
    fwrite(points.data(), 8, points.size(), g);
    fwrite(status.data(), 1, status.size(), g);
    fwrite(iterations.data(), 4, iterations.size(), g);
  }
  fclose(g);
  osfm_ctx_destroy(ctx);
  return rc == 0 ? 0 : 1;
}
