// undistort_main.cpp -- a stand-alone program around the host-emulated undistortion kernels (tests/native/build_undistort_emu.py links it
// with undistort.hip and emu_ctx.cpp under -fsanitize=address,undefined): reads one problem from a file, runs the remap through the given
// maps, the camera mapping, the fused undistortion and a batch of two, tries the refusals, and writes the results.  TEST INFRASTRUCTURE ONLY.
//
// file (little endian): int32 w, h, channels, map_w, map_h, out_w, out_h, interpolation, border, from_model, to_model, pad;
//   double from_params[16], to_params[16]; uint8 src[w * h * channels]; float map1[map_w * map_h], map2[map_w * map_h]
// output: uint8 remapped[map_w * map_h * channels]  (through the given maps, unscaled);
//   float cam1[w * h], cam2[w * h]                  (osfm_camera_mapping);
//   uint8 fused[out_w * out_h * channels]           (osfm_undistort_images, scaled to out_w x out_h);
//   uint8 batch[2][out_w * out_h * channels]        (the same image twice in one osfm_undistort_images call)
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
  int32_t head[12];
  double from_params[16], to_params[16];
  if (fread(head, 4, 12, f) != 12 || fread(from_params, 8, 16, f) != 16 || fread(to_params, 8, 16, f) != 16) return 2;
  const int32_t w = head[0], h = head[1], channels = head[2], map_w = head[3], map_h = head[4], out_w = head[5], out_h = head[6];
  const int interpolation = head[7], border = head[8];
  const int32_t from_model = head[9], to_model = head[10];
  std::vector<uint8_t> src((size_t)w * h * channels);
  std::vector<float> map1((size_t)map_w * map_h), map2((size_t)map_w * map_h);
  if (fread(src.data(), 1, src.size(), f) != src.size() || fread(map1.data(), 4, map1.size(), f) != map1.size() ||
      fread(map2.data(), 4, map2.size(), f) != map2.size())
    return 2;
  fclose(f);
  osfm_ctx *ctx = nullptr;
  if (osfm_ctx_create(0, &ctx) != OSFM_OK) return 3;
  FILE *g = fopen(argv[2], "wb");
  if (!g) return 2;
  int rc = 0, bad = 0;
  double ms = 0.0;
  const uint8_t *src_ptr[2] = {src.data(), src.data()};
  const int32_t ws[2] = {w, w}, hs[2] = {h, h}, cs[2] = {channels, channels}, ows[2] = {out_w, out_w}, ohs[2] = {out_h, out_h};
  {
    std::vector<uint8_t> out((size_t)map_w * map_h * channels);
    const float *m1[1] = {map1.data()}, *m2[1] = {map2.data()};
    uint8_t *dst[1] = {out.data()};
    rc = osfm_remap_images(ctx, 1, src_ptr, ws, hs, cs, m1, m2, &map_w, &map_h, &map_w, &map_h, interpolation, border, dst, &ms);
    if (rc != OSFM_OK) fprintf(stderr, "remap: %d %s\n", rc, osfm_last_error());
    fwrite(out.data(), 1, out.size(), g);
  }
  if (rc == OSFM_OK) {
    std::vector<float> cam1((size_t)w * h), cam2((size_t)w * h);
    float *m1[1] = {cam1.data()}, *m2[1] = {cam2.data()};
    rc = osfm_camera_mapping(ctx, 1, &from_model, from_params, &to_model, to_params, &w, &h, m1, m2, &ms);
    if (rc != OSFM_OK) fprintf(stderr, "mapping: %d %s\n", rc, osfm_last_error());
    fwrite(cam1.data(), 4, cam1.size(), g);
    fwrite(cam2.data(), 4, cam2.size(), g);
  }
  const int32_t cam_of[2] = {0, 0};
  for (int n = 1; n <= 2 && rc == OSFM_OK; n++) {
    std::vector<uint8_t> a((size_t)out_w * out_h * channels), b(a.size());
    uint8_t *dst[2] = {a.data(), b.data()};
    rc = osfm_undistort_images(ctx, n, src_ptr, ws, hs, cs, cam_of, 1, &from_model, from_params, &to_model, to_params, ows, ohs, interpolation, dst,
                               &ms);
    if (rc != OSFM_OK) fprintf(stderr, "undistort (%d): %d %s\n", n, rc, osfm_last_error());
    fwrite(a.data(), 1, a.size(), g);
    if (n == 2) fwrite(b.data(), 1, b.size(), g);
  }
  if (rc == OSFM_OK) {  // refusals leave the output alone; an empty batch succeeds
    std::vector<uint8_t> out((size_t)out_w * out_h * channels, 0xA5);
    uint8_t *dst[1] = {out.data()};
    const int32_t two = 2, wide = 40000, stranger = 1;
    bad += osfm_undistort_images(ctx, 1, src_ptr, ws, hs, &two, cam_of, 1, &from_model, from_params, &to_model, to_params, ows, ohs, interpolation, dst,
                                 nullptr) != OSFM_E_INVALID;
    bad += osfm_undistort_images(ctx, 1, src_ptr, ws, hs, cs, cam_of, 1, &from_model, from_params, &to_model, to_params, &wide, ohs, interpolation, dst,
                                 nullptr) != OSFM_E_INVALID;
    bad += osfm_undistort_images(ctx, 1, src_ptr, ws, hs, cs, &stranger, 1, &from_model, from_params, &to_model, to_params, ows, ohs, interpolation,
                                 dst, nullptr) != OSFM_E_INVALID;
    bad += osfm_undistort_images(ctx, 1, src_ptr, ws, hs, cs, cam_of, 1, &from_model, from_params, &to_model, to_params, ows, ohs, 7, dst, nullptr) !=
           OSFM_E_INVALID;
    bad += osfm_undistort_images(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 interpolation, nullptr, nullptr) != OSFM_OK;
    for (uint8_t v : out) bad += v != 0xA5;
    if (bad) fprintf(stderr, "refusals: %d unexpected results\n", bad);
  }
  fclose(g);
  osfm_ctx_destroy(ctx);
  return rc == 0 && bad == 0 ? 0 : 1;
}
