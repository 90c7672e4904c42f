// krcn_lanczos_f64.hip — the f64 instantiation of the device Lanczos recurrence.
#include "krcn_lanczos_impl.hpp"

krcn_status lanczos_f64(krcn_csr* h, const double* w, const double* g, int m, int reorth, double tol, double l2,
                        double* V, double* alphas_host, double* betas_host, krcn_lanczos_info* info, hipStream_t s,
                        bool enqueue_only) {
  return lanczos_impl<double>(h, w, g, m, reorth, tol, l2, V, alphas_host, betas_host, info, s, enqueue_only);
}

krcn_status cgs2_f64(krcn_csr* h, int k, const double* V, double* z, double* norm2_host, int* path_host, hipStream_t s) {
  return cgs2_impl<double>(h, k, V, z, norm2_host, path_host, s);
}

#ifdef KRCN_WIN_TIMING
extern "C" int krcn_debug_win_stamps_lz64(unsigned long long* out, int n, int reset) {
  return krcn::win_stamps_read(out, n, reset);
}
#endif
