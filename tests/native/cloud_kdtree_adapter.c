/* cloud_kdtree_adapter.c -- TEST INFRASTRUCTURE: the per-point neighbour averages of RemoveIsolatedPoints (sfm/src/map_helpers.cc:172-206)
 * through the reference's vendored vl/kdtree.c, compiled at test time from where the reference lies (tests/test_cloud_host.py), so that the
 * float32 brute-force restatement of tests/cloud_cases.py can be compared with the kd-tree bit for bit.  No reference source is copied:
 * this file only calls vlfeat's public kd-tree interface the way that function does. */
#include <math.h>
#include <stdlib.h>
#include <vl/kdtree.h>

int ref_isolation_averages(const double *positions, int n, int k, double *avg) {
  float *pos = (float *)malloc(sizeof(float) * 3 * (size_t)n);
  VlKDForestNeighbor *neighbors = (VlKDForestNeighbor *)malloc(sizeof(VlKDForestNeighbor) * (size_t)(k + 1));
  VlKDForest *forest;
  int i, j;
  if (!pos || !neighbors) return -1;
  for (i = 0; i < 3 * n; i++) pos[i] = (float)positions[i];
  forest = vl_kdforest_new(VL_TYPE_FLOAT, 3, 1, VlDistanceL2);
  vl_kdforest_build(forest, (vl_size)n, pos);
  for (i = 0; i < n; i++) {
    double sum = 0.0;
    int found = 0;
    vl_kdforest_query(forest, neighbors, (vl_size)(k + 1), pos + 3 * i);
    for (j = 1; j < k + 1; j++)
      if (isfinite(neighbors[j].distance)) {
        sum += neighbors[j].distance;
        found++;
      }
    avg[i] = found > 0 ? sum / found : 0.0;
  }
  vl_kdforest_delete(forest);
  free(neighbors);
  free(pos);
  return 0;
}
