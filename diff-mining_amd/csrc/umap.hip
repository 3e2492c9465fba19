// umap.hip — the C ABI of the UMAP projection below DM_UMAP_MAX_N rows: dm_umap_knn, dm_umap_graph (through the dense
// n x n graph) and dm_umap_layout.  The kernels and what they share with the route above that size are in umap_device.h.
#include "umap_device.h"

using namespace dm;

extern "C" {

int dm_umap_workspace_bytes(int n, int d, int n_neighbors, int n_components, size_t* bytes_out) {
    if (!bytes_out) return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors)) return rc;
    if (n_components < 1 || n_components > DM_UMAP_MAX_COMPONENTS) return DM_UMAP_E_COMPONENTS;
    if (d < 1) return DM_UMAP_E_D;
    *bytes_out = um_layout(nullptr, n, n_components, (size_t)2 * n * n_neighbors).bytes;
    return 0;
}

int dm_umap_knn(void* stream, const void* X, int n, int d, int n_neighbors, void* work, size_t work_bytes, int32_t* idx_out,
                float* dist_out) {
    if (!X || !work || !idx_out || !dist_out) return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors)) return rc;
    if (d < 1) return DM_UMAP_E_D;
    if (work_bytes < um_layout(nullptr, n, 1, (size_t)2 * n * n_neighbors).bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    UM_LAUNCH(umap_knn_kernel, dim3((n + kKnnRows - 1) / kKnnRows), dim3(kKnnThreads), (size_t)kKnnRows * n * sizeof(float),
              (const float*)X, n, d, n_neighbors, idx_out, dist_out);
    return 0;
}

int dm_umap_graph(void* stream, const int32_t* idx, const float* dist, int n, int n_neighbors, int n_epochs, void* work,
                  size_t work_bytes, float* rho_out, float* sigma_out, float* dense_P_out, int32_t* row_ptr_out, int32_t* col_out,
                  float* weight_out, int32_t* n_edges_out) {
    if (!idx || !dist || !work || !rho_out || !sigma_out || !dense_P_out || !row_ptr_out || !col_out || !weight_out || !n_edges_out)
        return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors)) return rc;
    if (n_epochs < 1) return DM_UMAP_E_EPOCHS;
    const size_t capacity = (size_t)2 * n * n_neighbors;
    const UmWork w = um_layout(work, n, 1, capacity);
    if (work_bytes < w.bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.A, 0, (size_t)n * n * sizeof(float), s) != hipSuccess) return DM_UMAP_E_HIP;
    UM_LAUNCH(umap_smooth_kernel<true>, dim3(row_blocks(n)), dim3(kRowWaves * kWave), 0, idx, dist, n, n_neighbors, rho_out, sigma_out, w.A);
    UM_LAUNCH(umap_union_kernel, dim3(n), dim3(256), 0, w.A, n, dense_P_out, w.rowmax);
    UM_LAUNCH(umap_prune_kernel, dim3(n), dim3(256), 0, dense_P_out, w.rowmax, n, n_epochs, w.rowcount);
    UM_LAUNCH(umap_scan_kernel, dim3(1), dim3(kScanThreads), 0, w.rowcount, n, row_ptr_out, n_edges_out);
    UM_LAUNCH(umap_compact_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), 0, dense_P_out, row_ptr_out, n, capacity, col_out,
              weight_out);
    return 0;
}

int dm_umap_layout(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_edges, int n_components,
                   float a, float b, int n_epochs, int seed, int first_epoch, int last_epoch, float* Y_inout, void* work,
                   size_t work_bytes) {
    return um_run_layout(stream, row_ptr, col, weight, n, n_edges, n_components, a, b, n_epochs, seed, first_epoch, last_epoch, Y_inout,
                         work, work_bytes, DM_UMAP_MAX_N);
}

}  // extern "C"
