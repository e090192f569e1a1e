// depthmap_main.cpp -- a stand-alone program around the host-emulated depthmap kernels (tests/native/build_depthmap_emu.py links it with
// depthmap.hip and emu_ctx.cpp under -fsanitize=address,undefined): reads one problem from a file, runs the three estimator methods and
// the cleaner and writes the results.  TEST INFRASTRUCTURE ONLY.
//
// file (little endian): int32 n_views, patch_size, iterations, num_planes; double min_depth, max_depth; uint64 seed; then per view
//   int32 w, h; double K[9], R[9], t[3]; uint8 image[w * h]; uint8 mask[w * h]
// output: per method 0, 1, 2: float depth[w0 * h0], plane[3 w0 h0], score[w0 h0]; int32 nghbr[w0 h0]; then float clean[w0 h0] of the
//   cleaner over the views' images read as depths (same_depth_threshold 0.5, min_consistent_views 2)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "osfm_mi355.h"

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s problem.bin result.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[4];
  double range[2];
  uint64_t seed;
  if (fread(head, 4, 4, f) != 4 || fread(range, 8, 2, f) != 2 || fread(&seed, 8, 1, f) != 1) return 2;
  const int n_views = head[0];
  std::vector<double> K((size_t)n_views * 9), R((size_t)n_views * 9), t((size_t)n_views * 3);
  std::vector<int32_t> widths((size_t)n_views), heights((size_t)n_views);
  std::vector<std::vector<uint8_t>> images((size_t)n_views), masks((size_t)n_views);
  std::vector<std::vector<float>> depths((size_t)n_views);
  for (int v = 0; v < n_views; v++) {
    int32_t wh[2];
    if (fread(wh, 4, 2, f) != 2 || fread(&K[9 * v], 8, 9, f) != 9 || fread(&R[9 * v], 8, 9, f) != 9 || fread(&t[3 * v], 8, 3, f) != 3) return 2;
    widths[v] = wh[0];
    heights[v] = wh[1];
    const size_t px = (size_t)wh[0] * wh[1];
    images[v].resize(px);
    masks[v].resize(px);
    if (px && (fread(images[v].data(), 1, px, f) != px || fread(masks[v].data(), 1, px, f) != px)) return 2;
    depths[v].assign(images[v].begin(), images[v].end());
  }
  fclose(f);
  std::vector<const uint8_t *> image_ptr, mask_ptr;
  std::vector<const float *> depth_ptr;
  for (int v = 0; v < n_views; v++) {
    image_ptr.push_back(images[v].data());
    mask_ptr.push_back(masks[v].data());
    depth_ptr.push_back(depths[v].data());
  }
  const int32_t offsets[2] = {0, n_views};
  const size_t px = n_views ? (size_t)widths[0] * heights[0] : 0;
  osfm_depthmap_params p;
  osfm_depthmap_params_default(&p);
  p.patch_size = head[1];
  p.patchmatch_iterations = head[2];
  p.num_depth_planes = head[3];
  osfm_ctx *ctx = nullptr;
  if (osfm_ctx_create(0, &ctx) != OSFM_OK) return 3;
  FILE *g = fopen(argv[2], "wb");
  if (!g) return 2;
  int rc = 0;
  for (int method = 0; method < 3 && rc == 0; method++) {
    std::vector<float> depth(px), plane(3 * px), score(px);
    std::vector<int32_t> nghbr(px);
    float *depth_out[1] = {depth.data()}, *plane_out[1] = {plane.data()}, *score_out[1] = {score.data()};
    int32_t *nghbr_out[1] = {nghbr.data()};
    double ms = 0.0;
    p.method = method;
    rc = osfm_depthmap_estimate(ctx, 1, offsets, K.data(), R.data(), t.data(), image_ptr.data(), mask_ptr.data(), widths.data(), heights.data(),
                                &range[0], &range[1], &p, seed, depth_out, plane_out, score_out, nghbr_out, &ms);
    if (rc != OSFM_OK) {
      fprintf(stderr, "method %d: %d %s\n", method, rc, osfm_last_error());
      break;
    }
    fwrite(depth.data(), 4, depth.size(), g);
    fwrite(plane.data(), 4, plane.size(), g);
    fwrite(score.data(), 4, score.size(), g);
    fwrite(nghbr.data(), 4, nghbr.size(), g);
  }
  if (rc == 0) {
    std::vector<float> clean(px);
    float *clean_out[1] = {clean.data()};
    p.same_depth_threshold = 0.5;
    p.min_consistent_views = 2;
    rc = osfm_depthmap_clean(ctx, 1, offsets, K.data(), R.data(), t.data(), depth_ptr.data(), widths.data(), heights.data(), &p, clean_out, nullptr);
    if (rc != OSFM_OK) fprintf(stderr, "clean: %d %s\n", rc, osfm_last_error());
    fwrite(clean.data(), 4, clean.size(), g);
  }
  fclose(g);
  osfm_ctx_destroy(ctx);
  return rc == 0 ? 0 : 1;
}
