// undistort.hip -- image undistortion on gfx950: what opensfm/undistort.py does shot by shot on one CPU thread
// (pygeometry.compute_camera_mapping, then cv2.remap of the image, the mask and the segmentation, then scale_image; six
// render_perspective_view_of_a_panorama per panorama) for a batch of images in one call.
//
// The numerics live in undistort_core.h (device + host emulation); this file adds the lanes, the kernels and the C ABI.
//   und_map_kernel        map1 / map2 of a list of maps (camera mappings or panorama views);
//   und_remap_kernel      remap through stored maps, read at the output pixel or, when a scaled size is given, at the pixel cv2.resize
//                         (INTER_NEAREST) would keep: only the pixels that survive scale_image are computed;
//   und_undistort_kernel  the fused path: the map entry is computed in registers by the function und_map_kernel calls, narrowed to
//                         float and sampled; no map is stored.
// One lane per output pixel, grid (tiles, batch entry).  A workgroup covers 32 x 8 output pixels, each of its four wavefronts an 8 x 8
// tile, so that the taps a wavefront gathers lie in few cache lines; a lane reads and writes all channels of its pixel (four channels as one dword store, one or three as byte stores; taps are byte loads).  No LDS, no
// atomics, no cooperative launch.  A pixel's result never depends on the grid or on another batch entry: a batch gives, byte for byte,
// what single calls give.
#include <math.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "osfm_internal.h"
#include "undistort_core.h"

using namespace osfm_und;

namespace {

constexpr int kBlock = 256, kTileW = 32, kTileH = 8;
constexpr int kMaxBatch = 65535;  // the batch entry is the grid's y

// the pixel of lane `tid` in tile `tile` of an image w pixels wide; false outside w x h
__device__ __forceinline__ bool tile_pixel(int tile, int tid, int w, int h, int *X, int *Y) {
  const int tiles_x = (w + kTileW - 1) / kTileW;
  const int lane = tid & 63, wave = tid >> 6;
  *X = (tile % tiles_x) * kTileW + wave * 8 + (lane & 7);
  *Y = (tile / tiles_x) * kTileH + (lane >> 3);
  return *X < w && *Y < h;
}

inline int64_t tiles_of(int w, int h) { return (int64_t)((w + kTileW - 1) / kTileW) * ((h + kTileH - 1) / kTileH); }

__device__ __forceinline__ void sample_store(const RemapJob &J, float x, float y, int interpolation, int border, int X, int Y) {
  const size_t at = (size_t)Y * J.out_w + X;
  if (J.channels == 1) {
    uint8_t px[1];
    sample_pixel<1>(J.src, J.src_w, J.src_h, x, y, interpolation, border, px);
    J.dst[at] = px[0];
  } else if (J.channels == 3) {
    uint8_t px[3];
    sample_pixel<3>(J.src, J.src_w, J.src_h, x, y, interpolation, border, px);
    uint8_t *d = J.dst + 3 * at;
    d[0] = px[0];
    d[1] = px[1];
    d[2] = px[2];
  } else {
    uint8_t px[4];
    sample_pixel<4>(J.src, J.src_w, J.src_h, x, y, interpolation, border, px);
    uint32_t word;  // (every image starts on a 256-byte boundary of the arena)
    memcpy(&word, px, 4);
    *(uint32_t *)(J.dst + 4 * at) = word;
  }
}

__global__ __launch_bounds__(kBlock) void und_map_kernel(const MapJob *__restrict__ jobs, float *__restrict__ map1, float *__restrict__ map2) {
  const MapJob &J = jobs[blockIdx.y];
  int X, Y;
  if (!tile_pixel((int)blockIdx.x, (int)threadIdx.x, J.w, J.h, &X, &Y)) return;
  float x, y;
  map_pixel(J, X, Y, &x, &y);
  const size_t at = (size_t)J.off + (size_t)Y * J.w + X;
  map1[at] = x;
  map2[at] = y;
}

__global__ __launch_bounds__(kBlock) void und_remap_kernel(const RemapJob *__restrict__ jobs, int interpolation, int border) {
  const RemapJob &J = jobs[blockIdx.y];
  int X, Y;
  if (!tile_pixel((int)blockIdx.x, (int)threadIdx.x, J.out_w, J.out_h, &X, &Y)) return;
  const bool scaled = J.out_w != J.map_w || J.out_h != J.map_h;
  const int mx = scaled ? resize_index(X, J.out_w, J.map_w) : X, my = scaled ? resize_index(Y, J.out_h, J.map_h) : Y;
  const size_t at = (size_t)my * J.map_w + mx;
  sample_store(J, J.map1[at], J.map2[at], interpolation, border, X, Y);
}

__global__ __launch_bounds__(kBlock) void und_undistort_kernel(const RemapJob *__restrict__ jobs, const MapJob *__restrict__ maps,
                                                               int interpolation) {
  const RemapJob &J = jobs[blockIdx.y];
  int X, Y;
  if (!tile_pixel((int)blockIdx.x, (int)threadIdx.x, J.out_w, J.out_h, &X, &Y)) return;
  const bool scaled = J.out_w != J.map_w || J.out_h != J.map_h;
  const int mx = scaled ? resize_index(X, J.out_w, J.map_w) : X, my = scaled ? resize_index(Y, J.out_h, J.map_h) : Y;
  float x, y;
  map_pixel(maps[blockIdx.y], mx, my, &x, &y);
  sample_store(J, x, y, interpolation, kConstant, X, Y);
}

// ---- host side ----
inline bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

int check_side(int v, const char *what, int i, const char *who) {
  OSFM_REQUIRE(v >= 1, OSFM_E_INVALID, "%s: entry %d: %s %d is not positive", who, i, what, v);
  OSFM_REQUIRE(v <= kMaxSide, OSFM_E_INVALID, "%s: entry %d: %s %d is above %d", who, i, what, v, kMaxSide);
  return OSFM_OK;
}

int check_cameras(int n, const int32_t *model, const double *params, const char *side, const char *who) {
  OSFM_REQUIRE(model && params, OSFM_E_INVALID, "%s: null %s cameras", who, side);
  for (int c = 0; c < n; c++) {
    OSFM_REQUIRE(model[c] >= OSFM_CAMERA_PERSPECTIVE && model[c] <= OSFM_CAMERA_SPHERICAL, OSFM_E_INVALID, "%s: %s camera %d has model %d", who,
                 side, c, model[c]);
    for (int k = 0; k < 16; k++)
      OSFM_REQUIRE(finite_d(params[16 * (size_t)c + k]), OSFM_E_INVALID, "%s: %s camera %d: parameter %d is not finite", who, side, c, k);
  }
  return OSFM_OK;
}

int check_modes(int interpolation, int border, const char *who) {
  OSFM_REQUIRE(interpolation == kNearest || interpolation == kLinear || interpolation == kArea, OSFM_E_INVALID,
               "%s: unknown interpolation %d (OSFM_INTER_NEAREST, OSFM_INTER_LINEAR or OSFM_INTER_AREA)", who, interpolation);
  OSFM_REQUIRE(border == kConstant || border == kWrap, OSFM_E_INVALID, "%s: unknown border %d (OSFM_BORDER_CONSTANT or OSFM_BORDER_WRAP)", who,
               border);
  return OSFM_OK;
}

// a batch of zero succeeds without a launch (kernel_ms is written by successful calls only: a refused call touches no output)
int empty_batch(double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  return OSFM_OK;
}

Camera make_camera(int model, const double *par) {
  Camera c;
  memset(&c, 0, sizeof(c));
  c.model = model;
  memcpy(c.par, par, sizeof(c.par));
  return c;
}

// the maps of `jobs` (off filled here) into the caller's map1[i] / map2[i]
int run_maps(osfm_ctx *ctx, std::vector<MapJob> &jobs, float *const *map1, float *const *map2, double *kernel_ms) {
  size_t total = 0;
  int64_t max_tiles = 0;
  for (MapJob &J : jobs) {
    J.off = (int64_t)total;
    total += osfm_round256((size_t)J.w * J.h * sizeof(float)) / sizeof(float);
    if (tiles_of(J.w, J.h) > max_tiles) max_tiles = tiles_of(J.w, J.h);
  }
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_jobs = A.add<MapJob>(jobs.size());
  const auto d_map1 = A.add<float>(total), d_map2 = A.add<float>(total);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_jobs, jobs.data(), st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(und_map_kernel, dim3((unsigned)max_tiles, (unsigned)jobs.size()), dim3(kBlock), 0, st, d_jobs.get(), d_map1.get(), d_map2.get());
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  for (size_t i = 0; i < jobs.size(); i++) {
    const size_t bytes = (size_t)jobs[i].w * jobs[i].h * sizeof(float);
    OSFM_HIP(hipMemcpyAsync(map1[i], d_map1.get() + jobs[i].off, bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(map2[i], d_map2.get() + jobs[i].off, bytes, hipMemcpyDeviceToHost, st));
  }
  OSFM_HIP(hipStreamSynchronize(st));
  return osfm_kernel_ms(ctx, kernel_ms);
}

int mapping_call(osfm_ctx *ctx, int n_maps, const int32_t *from_model, const double *from_params, const int32_t *to_model, const double *to_params,
                 const double *rotations, const int32_t *src_w, const int32_t *src_h, const int32_t *widths, const int32_t *heights,
                 float *const *map1, float *const *map2, double *kernel_ms, const char *who) {
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_REQUIRE(n_maps >= 0 && n_maps <= kMaxBatch, OSFM_E_INVALID, "%s: n_maps %d is outside 0 .. %d", who, n_maps, kMaxBatch);
  if (n_maps == 0) return empty_batch(kernel_ms);
  OSFM_REQUIRE(widths && heights && map1 && map2, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_TRY(check_cameras(n_maps, from_model, from_params, "from", who));
  OSFM_TRY(check_cameras(n_maps, to_model, to_params, "to", who));
  std::vector<MapJob> jobs((size_t)n_maps);
  for (int i = 0; i < n_maps; i++) {
    OSFM_TRY(check_side(widths[i], "width", i, who));
    OSFM_TRY(check_side(heights[i], "height", i, who));
    OSFM_REQUIRE(map1[i] && map2[i], OSFM_E_INVALID, "%s: entry %d has no output", who, i);
    MapJob &J = jobs[(size_t)i];
    memset(&J, 0, sizeof(J));
    J.from = make_camera(from_model[i], from_params + 16 * (size_t)i);
    J.to = make_camera(to_model[i], to_params + 16 * (size_t)i);
    J.kind = rotations ? kPanoramaView : kCameraMapping;
    J.w = widths[i];
    J.h = heights[i];
    if (rotations) {
      OSFM_REQUIRE(src_w && src_h, OSFM_E_INVALID, "%s: null argument", who);
      OSFM_TRY(check_side(src_w[i], "panorama width", i, who));
      OSFM_TRY(check_side(src_h[i], "panorama height", i, who));
      for (int k = 0; k < 9; k++) {
        OSFM_REQUIRE(finite_d(rotations[9 * (size_t)i + k]), OSFM_E_INVALID, "%s: entry %d: the rotation is not finite", who, i);
        J.R[k] = rotations[9 * (size_t)i + k];
      }
      J.src_w = src_w[i];
      J.src_h = src_h[i];
    }
  }
  return run_maps(ctx, jobs, map1, map2, kernel_ms);
}

int check_images(int n, const uint8_t *const *src, const int32_t *src_w, const int32_t *src_h, const int32_t *channels, const int32_t *out_w,
                 const int32_t *out_h, uint8_t *const *dst, const char *who) {
  OSFM_REQUIRE(src && src_w && src_h && channels && out_w && out_h && dst, OSFM_E_INVALID, "%s: null argument", who);
  for (int i = 0; i < n; i++) {
    OSFM_REQUIRE(channels[i] == 1 || channels[i] == 3 || channels[i] == 4, OSFM_E_INVALID, "%s: image %d has %d channels (1, 3 or 4)", who, i,
                 channels[i]);
    OSFM_TRY(check_side(src_w[i], "width", i, who));
    OSFM_TRY(check_side(src_h[i], "height", i, who));
    OSFM_TRY(check_side(out_w[i], "output width", i, who));
    OSFM_TRY(check_side(out_h[i], "output height", i, who));
    OSFM_REQUIRE(src[i] && dst[i], OSFM_E_INVALID, "%s: image %d has no input or no output", who, i);
  }
  return OSFM_OK;
}

}  // namespace

extern "C" int osfm_camera_mapping(osfm_ctx *ctx, int n_maps, const int32_t *from_model, const double *from_params, const int32_t *to_model,
                                   const double *to_params, const int32_t *widths, const int32_t *heights, float *const *map1, float *const *map2,
                                   double *kernel_ms) {
  return mapping_call(ctx, n_maps, from_model, from_params, to_model, to_params, nullptr, nullptr, nullptr, widths, heights, map1, map2, kernel_ms,
                      "osfm_camera_mapping");
}

extern "C" int osfm_panorama_mapping(osfm_ctx *ctx, int n_maps, const int32_t *from_model, const double *from_params, const int32_t *to_model,
                                     const double *to_params, const double *rotations, const int32_t *src_w, const int32_t *src_h,
                                     const int32_t *widths, const int32_t *heights, float *const *map1, float *const *map2, double *kernel_ms) {
  const char *who = "osfm_panorama_mapping";
  OSFM_REQUIRE(n_maps <= 0 || rotations, OSFM_E_INVALID, "%s: null rotations", who);
  return mapping_call(ctx, n_maps, from_model, from_params, to_model, to_params, rotations, src_w, src_h, widths, heights, map1, map2, kernel_ms,
                      who);
}

extern "C" int osfm_remap_images(osfm_ctx *ctx, int n_images, const uint8_t *const *src, const int32_t *src_w, const int32_t *src_h,
                                 const int32_t *channels, const float *const *map1, const float *const *map2, const int32_t *map_w,
                                 const int32_t *map_h, const int32_t *out_w, const int32_t *out_h, int interpolation, int border,
                                 uint8_t *const *dst, double *kernel_ms) {
  const char *who = "osfm_remap_images";
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_REQUIRE(n_images >= 0 && n_images <= kMaxBatch, OSFM_E_INVALID, "%s: n_images %d is outside 0 .. %d", who, n_images, kMaxBatch);
  OSFM_TRY(check_modes(interpolation, border, who));
  if (n_images == 0) return empty_batch(kernel_ms);
  OSFM_TRY(check_images(n_images, src, src_w, src_h, channels, out_w, out_h, dst, who));
  OSFM_REQUIRE(map1 && map2 && map_w && map_h, OSFM_E_INVALID, "%s: null argument", who);
  std::vector<RemapJob> jobs((size_t)n_images);
  // a map that several images share (one camera, many shots) is uploaded once
  std::map<std::pair<const float *, const float *>, size_t> slot_of;
  std::vector<size_t> map_off, map_slot((size_t)n_images), src_off((size_t)n_images), dst_off((size_t)n_images);
  std::vector<int> map_owner;
  size_t map_floats = 0, src_bytes = 0, dst_bytes = 0;
  int64_t max_tiles = 0;
  for (int i = 0; i < n_images; i++) {
    OSFM_TRY(check_side(map_w[i], "map width", i, who));
    OSFM_TRY(check_side(map_h[i], "map height", i, who));
    OSFM_REQUIRE(map1[i] && map2[i], OSFM_E_INVALID, "%s: image %d has no map", who, i);
    RemapJob &J = jobs[(size_t)i];
    memset(&J, 0, sizeof(J));
    J.src_w = src_w[i];
    J.src_h = src_h[i];
    J.map_w = map_w[i];
    J.map_h = map_h[i];
    J.out_w = out_w[i];
    J.out_h = out_h[i];
    J.channels = channels[i];
    const auto key = std::make_pair(map1[i], map2[i]);
    auto it = slot_of.find(key);
    if (it != slot_of.end()) {
      const int o = map_owner[it->second];
      OSFM_REQUIRE(map_w[o] == map_w[i] && map_h[o] == map_h[i], OSFM_E_INVALID, "%s: images %d and %d share a map but not its size", who, o, i);
      map_slot[(size_t)i] = it->second;
    } else {
      map_slot[(size_t)i] = slot_of[key] = map_off.size();
      map_off.push_back(map_floats);
      map_owner.push_back(i);
      map_floats += osfm_round256((size_t)map_w[i] * map_h[i] * sizeof(float)) / sizeof(float);
    }
    src_off[(size_t)i] = src_bytes;
    src_bytes += osfm_round256((size_t)J.src_w * J.src_h * J.channels);
    dst_off[(size_t)i] = dst_bytes;
    dst_bytes += osfm_round256((size_t)J.out_w * J.out_h * J.channels);
    if (tiles_of(J.out_w, J.out_h) > max_tiles) max_tiles = tiles_of(J.out_w, J.out_h);
  }
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_jobs = A.add<RemapJob>(jobs.size());
  const auto d_map1 = A.add<float>(map_floats), d_map2 = A.add<float>(map_floats);
  const auto d_src = A.add<uint8_t>(src_bytes), d_dst = A.add<uint8_t>(dst_bytes);
  OSFM_HIP(A.alloc(ctx));
  for (size_t s = 0; s < map_off.size(); s++) {
    const int o = map_owner[s];
    const size_t bytes = (size_t)map_w[o] * map_h[o] * sizeof(float);
    OSFM_HIP(hipMemcpyAsync(d_map1.get() + map_off[s], map1[o], bytes, hipMemcpyHostToDevice, st));
    OSFM_HIP(hipMemcpyAsync(d_map2.get() + map_off[s], map2[o], bytes, hipMemcpyHostToDevice, st));
  }
  for (int i = 0; i < n_images; i++) {
    RemapJob &J = jobs[(size_t)i];
    J.src = d_src.get() + src_off[(size_t)i];
    J.dst = d_dst.get() + dst_off[(size_t)i];
    J.map1 = d_map1.get() + map_off[map_slot[(size_t)i]];
    J.map2 = d_map2.get() + map_off[map_slot[(size_t)i]];
    OSFM_HIP(hipMemcpyAsync(d_src.get() + src_off[(size_t)i], src[i], (size_t)J.src_w * J.src_h * J.channels, hipMemcpyHostToDevice, st));
  }
  OSFM_HIP(A.upload(d_jobs, jobs.data(), st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(und_remap_kernel, dim3((unsigned)max_tiles, (unsigned)n_images), dim3(kBlock), 0, st, d_jobs.get(),
                     interpolation == kNearest ? (int)kNearest : (int)kLinear, border);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  for (int i = 0; i < n_images; i++)
    OSFM_HIP(hipMemcpyAsync(dst[i], d_dst.get() + dst_off[(size_t)i], (size_t)out_w[i] * out_h[i] * channels[i], hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  return osfm_kernel_ms(ctx, kernel_ms);
}

extern "C" int osfm_undistort_images(osfm_ctx *ctx, int n_images, const uint8_t *const *src, const int32_t *widths, const int32_t *heights,
                                     const int32_t *channels, const int32_t *image_cam, int n_cams, const int32_t *from_model,
                                     const double *from_params, const int32_t *to_model, const double *to_params, const int32_t *out_w,
                                     const int32_t *out_h, int interpolation, uint8_t *const *dst, double *kernel_ms) {
  const char *who = "osfm_undistort_images";
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_REQUIRE(n_images >= 0 && n_images <= kMaxBatch && n_cams >= 0, OSFM_E_INVALID, "%s: n_images %d is outside 0 .. %d, or n_cams < 0", who,
               n_images, kMaxBatch);
  OSFM_TRY(check_modes(interpolation, kConstant, who));
  if (n_images == 0) return empty_batch(kernel_ms);
  OSFM_TRY(check_images(n_images, src, widths, heights, channels, out_w, out_h, dst, who));
  OSFM_REQUIRE(image_cam, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_TRY(check_cameras(n_cams, from_model, from_params, "from", who));
  OSFM_TRY(check_cameras(n_cams, to_model, to_params, "to", who));
  for (int i = 0; i < n_images; i++)
    OSFM_REQUIRE(image_cam[i] >= 0 && image_cam[i] < n_cams, OSFM_E_INVALID, "%s: image %d names a camera outside the table", who, i);
  std::vector<RemapJob> jobs((size_t)n_images);
  std::vector<MapJob> maps((size_t)n_images);
  std::vector<size_t> src_off((size_t)n_images), dst_off((size_t)n_images);
  size_t src_bytes = 0, dst_bytes = 0;
  int64_t max_tiles = 0;
  for (int i = 0; i < n_images; i++) {
    RemapJob &J = jobs[(size_t)i];
    memset(&J, 0, sizeof(J));
    J.src_w = J.map_w = widths[i];
    J.src_h = J.map_h = heights[i];
    J.out_w = out_w[i];
    J.out_h = out_h[i];
    J.channels = channels[i];
    MapJob &M = maps[(size_t)i];
    memset(&M, 0, sizeof(M));
    M.from = make_camera(from_model[image_cam[i]], from_params + 16 * (size_t)image_cam[i]);
    M.to = make_camera(to_model[image_cam[i]], to_params + 16 * (size_t)image_cam[i]);
    M.kind = kCameraMapping;
    M.w = widths[i];
    M.h = heights[i];
    src_off[(size_t)i] = src_bytes;
    src_bytes += osfm_round256((size_t)J.src_w * J.src_h * J.channels);
    dst_off[(size_t)i] = dst_bytes;
    dst_bytes += osfm_round256((size_t)J.out_w * J.out_h * J.channels);
    if (tiles_of(J.out_w, J.out_h) > max_tiles) max_tiles = tiles_of(J.out_w, J.out_h);
  }
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_jobs = A.add<RemapJob>(jobs.size());
  const auto d_maps = A.add<MapJob>(maps.size());
  const auto d_src = A.add<uint8_t>(src_bytes), d_dst = A.add<uint8_t>(dst_bytes);
  OSFM_HIP(A.alloc(ctx));
  for (int i = 0; i < n_images; i++) {
    RemapJob &J = jobs[(size_t)i];
    J.src = d_src.get() + src_off[(size_t)i];
    J.dst = d_dst.get() + dst_off[(size_t)i];
    OSFM_HIP(hipMemcpyAsync(d_src.get() + src_off[(size_t)i], src[i], (size_t)J.src_w * J.src_h * J.channels, hipMemcpyHostToDevice, st));
  }
  OSFM_HIP(A.upload(d_jobs, jobs.data(), st));
  OSFM_HIP(A.upload(d_maps, maps.data(), st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(und_undistort_kernel, dim3((unsigned)max_tiles, (unsigned)n_images), dim3(kBlock), 0, st, d_jobs.get(), d_maps.get(),
                     interpolation == kNearest ? (int)kNearest : (int)kLinear);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  for (int i = 0; i < n_images; i++)
    OSFM_HIP(hipMemcpyAsync(dst[i], d_dst.get() + dst_off[(size_t)i], (size_t)out_w[i] * out_h[i] * channels[i], hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  return osfm_kernel_ms(ctx, kernel_ms);
}
