// bank_keypoints_plan_probe.hip - the plan of a bank key-point query next to the bank query's, without a GPU
// (tests/test_bank_keypoints_cpu.py).
//
// A stand-alone host program, compiled host-only like base_motion_plan_probe.hip: it runs the library's planner
// (plan_simulate, kr_plan.hip) on a matrix of bank queries, once for a bank source and once for a bank key-point source
// (SimSrc::kind), and prints one line per query and form:
// "<label> | bank|bankkp | rc path family W occ nn overlap smem0 smem1 | why".  The test compares the two forms field by
// field; a refusal's text must name its own call.
#define KR_MS_NO_INST
#include "kr_plan.hip"

#include <cstdio>
#include <string>

namespace kr {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t, const char* what) { g_err = what; return KR_E_HIP; }
}  // namespace kr

// net: 0 = 28 -> 64 -> 64 -> 25, 1 = 28 -> 64 -> 25, 2 = a shape the persistent kernel does not evaluate (no JVP form)
template <typename T>
static void set_net(kr::MlpDev<T>& M, int net) {
  M = kr::MlpDev<T>{};
  M.n_layers = net == 1 ? 2 : 3;
  M.dims[0] = 28; M.dims[1] = 64; M.dims[2] = net == 1 ? 25 : 64; M.dims[3] = 25;
  M.max_dim = 64;
  M.mfma_ok = true;
  M.jvp_ok = net != 2;
}

struct Opt { const char* name; int val; };

template <typename T>
static void run(const char* dt, int N, long long B, int scheme, int net, const Opt& o) {
  for (int form = 0; form < 2; ++form) {
    kr_handle h = kr_handle{};
    h.lds_limit = 160 * 1024;
    h.params.N = N;
    h.cf.N = h.cd.N = N;
    h.cf.diag = h.cd.diag = 1;
    h.mfma_mlp = 1;
    const std::string on = o.name ? o.name : "";
    if (on == "overlap") h.overlap = o.val;
    else if (on == "waves_per_rod") h.waves_per_rod = o.val;
    else if (on == "persistent") h.persistent = o.val;
    else if (on == "ms_mode") h.ms_mode = o.val;
    else if (on == "ms_batch_limit") h.ms_batch_limit = o.val;
    else if (on == "lds_limit") h.lds_limit = o.val;
    else if (on == "mfma_mlp") h.mfma_mlp = o.val;
    kr_param_table t;
    t.N = N;
    kr_mlp_bank bank;
    bank.K = 3;
    set_net(bank.mf, net); set_net(bank.md, net);
    kr::SimSrc src;
    src.kind = form ? kr::KR_SRC_BANK_KEYPOINTS : kr::KR_SRC_BANK;
    src.table = &t;
    src.bank = &bank;
    const kr::SimPlan p = kr::plan_simulate<T>(&h, kr::plan_query(src, B, 2, scheme, 1));
    std::printf("%s,%d,%lld,%c,n%d,%s=%d | %s | %d %d %d %d %d %d %d %zu %zu | %s\n", dt, N, B, scheme == KR_EULER ? 'E' : 'R', net,
                o.name ? o.name : "none", o.val, form ? "bankkp" : "bank", p.rc, p.path, (int)p.family, p.W, p.occ, (int)p.nn, (int)p.overlap,
                p.smem[0], p.smem[1], p.why);
  }
}

int main() {
  const Opt opts[] = {{nullptr, 0}, {"ms_mode", 0}, {"persistent", 0}, {"ms_batch_limit", 4}, {"waves_per_rod", 2}, {"overlap", 0},
                      {"lds_limit", 16384}, {"mfma_mlp", 0}};
  for (int N : {8, 9, 10, 20, 23, 100, 128, 129})
    for (long long B : {6LL, 2048LL})
      for (int scheme : {(int)KR_EULER, (int)KR_RK4})
        for (int net : {0, 1, 2})
          for (const Opt& o : opts) {
            run<double>("f64", N, B, scheme, net, o);
            run<float>("f32", N, B, scheme, net, o);
          }
  return 0;
}
