// prune_main.cpp -- a stand-alone program around the host-emulated pruning kernels (tests/native/build_prune_emu.py links it with
// prune.hip and emu_ctx.cpp under -fsanitize=address,undefined): reads a batch from a file, runs osfm_depthmap_prune with buffers of
// exactly `capacity` rows, then once more with one row less than the batch keeps (the refusal), and writes the results.
// TEST INFRASTRUCTURE ONLY.
//
// file (little endian): int32 n_problems; double same_depth_threshold; int64 capacity; int32 view_offsets[n_problems + 1]; then per view
//   int32 w, h; double K[9], R[9], t[3]; float depth[w h]; float plane[3 w h]; uint8 color[3 w h]; uint8 label[w h]
// output: int64 counts[n_problems]; with n their sum: float points[3 n], normals[3 n]; uint8 colors[3 n], labels[n];
//   int32 status of the refused call (OSFM_OK when the batch keeps no row: there is nothing to refuse); int64 its counts[n_problems]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "osfm_mi355.h"

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s batch.bin result.bin\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_problems;
  double threshold;
  int64_t capacity;
  if (fread(&n_problems, 4, 1, f) != 1 || fread(&threshold, 8, 1, f) != 1 || fread(&capacity, 8, 1, f) != 1 || n_problems < 0 || capacity < 0) return 2;
  std::vector<int32_t> offsets((size_t)n_problems + 1);
  if (fread(offsets.data(), 4, offsets.size(), f) != offsets.size()) return 2;
  const int n_views = offsets[(size_t)n_problems];
  std::vector<double> K((size_t)n_views * 9), R((size_t)n_views * 9), t((size_t)n_views * 3);
  std::vector<int32_t> widths((size_t)n_views), heights((size_t)n_views);
  std::vector<std::vector<float>> depths((size_t)n_views), planes((size_t)n_views);
  std::vector<std::vector<uint8_t>> colors((size_t)n_views), labels((size_t)n_views);
  for (int v = 0; v < n_views; v++) {
    int32_t wh[2];
    if (fread(wh, 4, 2, f) != 2 || fread(&K[9 * v], 8, 9, f) != 9 || fread(&R[9 * v], 8, 9, f) != 9 || fread(&t[3 * v], 8, 3, f) != 3) return 2;
    widths[v] = wh[0];
    heights[v] = wh[1];
    const size_t px = (size_t)wh[0] * wh[1];
    depths[v].resize(px);
    planes[v].resize(3 * px);
    colors[v].resize(3 * px);
    labels[v].resize(px);
    if (px && (fread(depths[v].data(), 4, px, f) != px || fread(planes[v].data(), 4, 3 * px, f) != 3 * px ||
               fread(colors[v].data(), 1, 3 * px, f) != 3 * px || fread(labels[v].data(), 1, px, f) != px))
      return 2;
  }
  fclose(f);
  std::vector<const float *> depth_ptr, plane_ptr;
  std::vector<const uint8_t *> color_ptr, label_ptr;
  for (int v = 0; v < n_views; v++) {
    depth_ptr.push_back(depths[v].data());
    plane_ptr.push_back(planes[v].data());
    color_ptr.push_back(colors[v].data());
    label_ptr.push_back(labels[v].data());
  }
  osfm_depthmap_params p = osfm_depthmap_params();  // (the pruner reads same_depth_threshold alone)
  p.same_depth_threshold = threshold;
  osfm_ctx *ctx = nullptr;
  if (osfm_ctx_create(0, &ctx) != OSFM_OK) return 3;
  // exactly `capacity` rows: a row written past them is a heap overflow the sanitizer reports
  std::vector<float> points(3 * (size_t)capacity), normals(3 * (size_t)capacity);
  std::vector<uint8_t> out_colors(3 * (size_t)capacity), out_labels((size_t)capacity);
  std::vector<int64_t> counts((size_t)n_problems, -1), refused_counts((size_t)n_problems, -1);
  double ms = 0.0;
  int rc = osfm_depthmap_prune(ctx, n_problems, offsets.data(), K.data(), R.data(), t.data(), depth_ptr.data(), plane_ptr.data(), color_ptr.data(),
                               label_ptr.data(), widths.data(), heights.data(), &p, capacity, points.data(), normals.data(), out_colors.data(),
                               out_labels.data(), counts.data(), &ms);
  if (rc != OSFM_OK) {
    fprintf(stderr, "prune: %d %s\n", rc, osfm_last_error());
    osfm_ctx_destroy(ctx);
    return 1;
  }
  int64_t n = 0;
  for (int b = 0; b < n_problems; b++) n += counts[b];
  int32_t refused = OSFM_OK;
  if (n > 0) {
    std::vector<float> small_points(3 * (size_t)(n - 1)), small_normals(3 * (size_t)(n - 1));
    std::vector<uint8_t> small_colors(3 * (size_t)(n - 1)), small_labels((size_t)(n - 1));
    refused = osfm_depthmap_prune(ctx, n_problems, offsets.data(), K.data(), R.data(), t.data(), depth_ptr.data(), plane_ptr.data(), color_ptr.data(),
                                  label_ptr.data(), widths.data(), heights.data(), &p, n - 1, small_points.data(), small_normals.data(),
                                  small_colors.data(), small_labels.data(), refused_counts.data(), nullptr);
  } else {
    refused_counts = counts;
  }
  FILE *g = fopen(argv[2], "wb");
  if (!g) return 2;
  fwrite(counts.data(), 8, counts.size(), g);
  fwrite(points.data(), 4, 3 * (size_t)n, g);
  fwrite(normals.data(), 4, 3 * (size_t)n, g);
  fwrite(out_colors.data(), 1, 3 * (size_t)n, g);
  fwrite(out_labels.data(), 1, (size_t)n, g);
  fwrite(&refused, 4, 1, g);
  fwrite(refused_counts.data(), 8, refused_counts.size(), g);
  fclose(g);
  osfm_ctx_destroy(ctx);
  return 0;
}
