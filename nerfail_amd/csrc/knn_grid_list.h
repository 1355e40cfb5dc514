// The list form of the grid search (fg revision 1). The search kernel is a template in knn_grid.hip - the grid's layout (carve), the
// record of built workspaces and the kernel body live there and are not restated: knn_grid.hip instantiates the kernel for a
// compact query list and fg_scene.hip, which owns the entry point, calls this launcher.
#pragma once
#include "common.h"

namespace nerfail {

// knn8_grid_kernel<WEIGHTS, LIST> over queries[n,3] in the flat 64-queries-per-wave form: query j's weights and indices go to row
// pix[j] of the two planes of weight_and_index [2,n_rows,8]; then the one-wave fold of the per-wave partials (in `workspace`, one
// double per 64 queries) into *sum_d2 (NULL: neither). n = 0 launches no search and folds nothing into a 0.
// knn8_grid_list_check: what only knn_grid.hip can check - the grid workspace's size, the point count it was built for, the launch
// size - so that the entry point refuses before its first launch; the launcher repeats it, the caller checks everything else.
int knn8_grid_list_check(int64_t n, int64_t n_points, const void* grid_workspace, size_t grid_workspace_bytes);
int knn8_grid_weights_list_launch(const float* queries, int64_t n, const int32_t* pix, int64_t n_rows, int64_t n_points, float c,
                                  float* weight_and_index, double* sum_d2, const void* grid_workspace, size_t grid_workspace_bytes,
                                  void* workspace, hipStream_t s);

}  // namespace nerfail
