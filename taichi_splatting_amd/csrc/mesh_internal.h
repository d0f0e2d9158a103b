// mesh_internal.h — what the mesh files (mesh.hip, mesh_simplify.hip) share: the size limits of an indexed triangle
// mesh, the one-lane-per-item grid and the corner index test.
#pragma once

#include "common.h"

namespace ms {

__device__ __forceinline__ bool mesh_in_range(int32_t a, int32_t b, int32_t c, int32_t num_vertices) {
  return (uint32_t)a < (uint32_t)num_vertices && (uint32_t)b < (uint32_t)num_vertices && (uint32_t)c < (uint32_t)num_vertices;
}

static inline bool mesh_sizes_ok(int64_t num_vertices, int64_t num_faces) {
  return num_vertices >= 0 && num_faces >= 0 && num_vertices <= MS_MESH_MAX_VERTICES && num_faces <= MS_MESH_MAX_CORNERS / 3;
}
static inline dim3 mesh_grid(int64_t n) { return dim3((unsigned)div_up(n > 0 ? n : 1, 256)); }

}  // namespace ms
