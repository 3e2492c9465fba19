// umap_spectral.hip — the C ABI of UMAP's spectral initialisation below DM_UMAP_MAX_N rows.  The solver, and what it
// shares with the route above that size, is in umap_spectral_device.h.
#include "umap_spectral_device.h"

using namespace dm;

extern "C" {

int dm_umap_spectral_workspace_bytes(int n, int n_components, size_t* bytes_out) {
    return sp_workspace_bytes(n, n_components, bytes_out, DM_UMAP_MAX_N);
}

int dm_umap_spectral(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_components, int seed,
                     const float* noise, const float* fallback, void* work, size_t work_bytes, float* Y0_out, double* eigvals_out,
                     double* eigvecs_out, double* status_out) {
    return sp_run(stream, row_ptr, col, weight, n, n_components, seed, noise, fallback, work, work_bytes, Y0_out, eigvals_out, eigvecs_out,
                  status_out, DM_UMAP_MAX_N);
}

}  // extern "C"
