// kr_train_bank.hpp - a bank of independent trainings of one network shape (kr_train_bank_*): what kr_train.hip (the C
// ABI) asks of kr_mlp_fused.hip (the kernels and their launch code).
#pragma once
#include "kr_internal.hpp"

namespace kr {

struct BankNetDesc {  // one training; device pointers owned by the caller (kr_train_bank_net with Q = S * K)
  int64_t Q;
  float ds;
  float *p, *g, *m, *v;
  const float* lower;
  double* sched;
  const float *x, *base, *target_rows;
  float* loss_log;
};
struct BankStep {  // one kr_train_bank_epochs call
  int64_t n_epochs, step;
  double beta1, beta2, eps, weight_decay, factor, threshold, min_lr;
  int patience;
  int64_t log_offset;
  bool repack;
};
struct FusedBank;
// the shapes whose epoch kernels have bank forms (a subset of fused_mlp_supported)
bool fused_bank_shape_served(int n_layers, const int32_t* dims);
// arguments are checked by the caller (kr_train_bank_check); allocates and fills the bank's device memory, launches nothing
int fused_bank_create(int n_nets, const BankNetDesc* nets, int K, int n_layers, const int32_t* dims, const int32_t* acts,
                      float inv_denom, FusedBank** out);
int fused_bank_epochs(FusedBank* bank, const BankStep& st, hipStream_t s);
void fused_bank_destroy(FusedBank* bank);

}  // namespace kr
