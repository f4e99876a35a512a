// select_probe.hip - which kernels a call launches, checked without a GPU (tests/test_select_cpu.py).
//
// A stand-alone host program: compiled host-only, it runs the library's real planner (plan_simulate / plan_step,
// kr_plan.hip) and launchers against a launch plumbing that records instead of launching - the kernel's instantiation
// (dladdr + demangling of the address hipLaunchKernel gets), grid, block, dynamic LDS, which pointers of the
// SimArgs / StepArgs the launch code filled in, and whether every scalar member arrived as passed - and, read back from
// the handle, what note_sim_plan / note_step_plan wrote to last_sim_path / last_overlap / last_waves_per_rod.  One line
// per case of the matrix below; tests/golden/selection_parent.txt.gz holds the lines of the same matrix driven through
// the launcher interfaces this planner replaced.  The predictor-image members (pred_io / pred_load, pred / pred_reset)
// are the probe's own constants in those lines; what a simulate call puts there is plan_pred_image's decision, which the
// "pred" lines at the end print for test_select_cpu.py to compare with the rule of the parent's simulate_impl.
// The "src" lines drive the five table-family sources (table, bank, loads, boundary, key points) through launch_sim and
// also print the source struct as the kernel received it, read back from the launch's own arguments: every field the
// launcher fills is a distinct sentinel, so a dropped or swapped one shows (tests/golden/selection_parent_sources.txt.gz).
#define KR_MS_NO_INST
#include "kr_bank_impl.hpp"
#include "kr_load_impl.hpp"
#include "kr_bnd_impl.hpp"
#include "kr_kp_impl.hpp"
#include "kr_mswo_impl.hpp"
#include "kr_mswn_impl.hpp"
#include "kr_msn_impl.hpp"
#include "kr_plan.hip"

// ---- the HIP launch plumbing, replaced by recorders ----
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace kr {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t, const char* what) { g_err = what; return KR_E_HIP; }
int ensure_ws(kr_handle*, size_t) { return KR_OK; }
int ensure_resume(kr_handle*, int64_t) { return KR_OK; }
int ensure_hist_ws(kr_handle*, size_t) { return KR_OK; }
}  // namespace kr

static std::vector<std::string> g_launches;  // what the case under test launched (or readied), in order
static std::string g_expect;                 // scalar members of the SimArgs / StepArgs the case passed in
static const void* g_attr_kern = nullptr;    // kernel of the last hipFuncGetAttributes (prepare entries)
static dim3 g_grid, g_block;
static size_t g_smem;
static bool g_print_src = false;             // "src" lines: every launch also prints its source struct

static std::string kernel_name(const void* func) {
  Dl_info info;
  if (!dladdr(func, &info) || !info.dli_sname) return "?";
  int st = 0;
  char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
  std::string n = st == 0 && d ? d : info.dli_sname;
  std::free(d);
  std::string out;
  for (size_t i = 0; i < n.size(); ++i) {
    if (n[i] == ' ') continue;
    if (n.compare(i, 4, "kr::") == 0) { i += 3; continue; }
    out += n[i];
  }
  // (the default sources of the persistent kernels: the handle's constants and network)
  for (const char* d : {",RodConst<float>", ",RodConst<double>", ",MlpDev<float>", ",MlpDev<double>"})
    for (size_t at; (at = out.find(d)) != std::string::npos;) out.erase(at, std::strlen(d));
  // "void name<...>(parameters)" -> "name<...>"
  if (out.compare(0, 4, "void") == 0) out.erase(0, 4);
  int depth = 0;
  for (size_t i = 0; i < out.size(); ++i) {
    if (out[i] == '<') ++depth;
    else if (out[i] == '>') --depth;
    else if (out[i] == '(' && depth == 0) { out.erase(i); break; }
  }
  return out;
}

namespace kr {
int dyn_lds(const void* kern, size_t smem) {
  if (kern == g_attr_kern) g_launches.push_back("ready " + kernel_name(kern) + " " + std::to_string(smem));
  g_attr_kern = nullptr;
  return KR_OK;
}
}  // namespace kr

template <typename T>
static std::string sim_scalars(const kr::SimArgs<T>& a) {
  char b[400];
  std::snprintf(b, sizeof b, "B=%lld T=%lld slot=%lld ring=%d tol=%g tolA=%g fd=%g hc1=%g hc2=%g maxit=%d pred=%d rt=%d lowp=%d bo=%d pi=%d tip=%d st=%d",
                (long long)a.B, (long long)a.T_steps, (long long)a.slot_elems, a.ring, (double)a.tol, (double)a.tolA,
                (double)a.fd_eps, (double)a.hc1, (double)a.hc2, a.maxit, a.predictor, a.residual_test, a.nn_lowp,
                a.nn_base_only, a.prev_init != nullptr, a.tip != nullptr, a.status != nullptr);
  return b;
}
template <typename T>
static std::string step_scalars(const kr::StepArgs<T>& a) {
  char b[400];
  std::snprintf(b, sizeof b, "B=%lld ts=%lld tol=%g tolA=%g fd=%g hc1=%g hc2=%g maxit=%d mode=%d po=%d reset=%d hp=%d pl=%d rt=%d r=%d mid=%d",
                (long long)a.B, (long long)a.tens_stride, (double)a.tol, (double)a.tolA, (double)a.fd_eps, (double)a.hc1,
                (double)a.hc2, a.maxit, a.mode, a.pred_order, a.pred_reset, a.pred_has_prev, a.pred_limit,
                a.residual_test, a.r_out != nullptr, a.mid != nullptr);
  return b;
}
template <typename T>
static std::string sim_flags(const kr::SimArgs<T>& a) {
  char b[64];
  std::snprintf(b, sizeof b, "r%dh%dp%dl%d", a.resume != nullptr, a.hist_ws != nullptr, a.pred_io != nullptr, a.pred_load);
  std::string s = b, sc = sim_scalars(a);
  if (sc != g_expect) s += " ARGS{" + sc + "}";
  return s;
}
template <typename T>
static std::string step_flags(const kr::StepArgs<T>& a) {
  char b[64];
  std::snprintf(b, sizeof b, "w%dc%dp%d", a.hist_ws != nullptr, a.act_ws != nullptr, a.pred != nullptr);
  std::string s = b, sc = step_scalars(a);
  if (sc != g_expect) s += " ARGS{" + sc + "}";
  return s;
}

// The parameter source (first kernel argument) and, for a bank kernel, the network source (third) as the launch passed them
template <typename T>
static std::string src_fields(const std::string& n, void** args) {
  char b[320];
  const auto* t = static_cast<const kr::RodTable<T>*>(args[0]);
  int at = std::snprintf(b, sizeof b, " src{rows=%p N=%d", (const void*)t->rows, t->N);
  if (n.find("RodTableBndKp<") != std::string::npos) {
    const auto* k = static_cast<const kr::RodTableBndKp<T>*>(args[0]);
    at += std::snprintf(b + at, sizeof b - at, " bnd=%p kp=%p K=%d lo=%llx hi=%llx", (const void*)k->bnd, (const void*)k->kp, k->K, k->mask_lo, k->mask_hi);
  } else if (n.find("RodTableBnd<") != std::string::npos) {
    at += std::snprintf(b + at, sizeof b - at, " bnd=%p", (const void*)static_cast<const kr::RodTableBnd<T>*>(args[0])->bnd);
  } else if (n.find("RodTableLoads<") != std::string::npos) {
    at += std::snprintf(b + at, sizeof b - at, " loads=%p", (const void*)static_cast<const kr::RodTableLoads<T>*>(args[0])->loads);
  }
  if (n.find("MlpBank<") != std::string::npos) {
    const auto* k = static_cast<const kr::MlpBank<T>*>(args[2]);
    at += std::snprintf(b + at, sizeof b - at, " idx=%p stride=%llu layers=%d", (const void*)k->net_of_rod, k->stride, k->n_layers);
  }
  return std::string(b) + "}";
}

extern "C" {
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t smem, hipStream_t) {
  g_grid = grid; g_block = block; g_smem = smem;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* smem, hipStream_t* s) {
  *grid = g_grid; *block = g_block; *smem = g_smem; *s = nullptr;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* func, dim3 grid, dim3 block, void** args, size_t smem, hipStream_t) {
  const std::string n = kernel_name(func);
  char b[96];
  std::snprintf(b, sizeof b, " %ux%u %zu ", grid.x, block.x, smem);
  std::string s = n + b;
  const bool f64 = n.find("<double") != std::string::npos;
  if (n.find("sim_kernel<") != std::string::npos)
    s += f64 ? sim_flags(*static_cast<kr::SimArgs<double>*>(args[1])) : sim_flags(*static_cast<kr::SimArgs<float>*>(args[1]));
  else if (n.find("step_kernel<") != std::string::npos)
    s += f64 ? step_flags(*static_cast<kr::StepArgs<double>*>(args[1])) : step_flags(*static_cast<kr::StepArgs<float>*>(args[1]));
  else
    s += "-";
  if (g_print_src) s += f64 ? src_fields<double>(n, args) : src_fields<float>(n, args);
  g_launches.push_back(s);
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipFuncGetAttributes(hipFuncAttributes* fa, const void* kern) {
  std::memset(fa, 0, sizeof *fa);
  g_attr_kern = kern;
  return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { static void* m = nullptr; return &m; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned int, void*, void*, dim3*, dim3*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}

// ---- the matrix ----
enum Entry { E_SIM, E_STEP, E_RESID, E_TAB, E_BANK, E_PREP, E_LOADS, E_BND, E_KP };
static const char* const kEntryName[] = {"sim", "step", "resid", "tab", "bank", "prep", "loads", "bnd", "kp"};
// network: 0 none; 1 served three-layer (mfma_ok, jvp_ok); 2 mfma_ok without jvp_ok; 3 neither; 4 nn_input_history = 1;
// 5 use_nn with no network set.  Bank entries: the bank's network 0 has the flags of kind 1 / 2 / 3
struct Case {
  bool f64;
  int N;
  int64_t B;
  int scheme, diag, net, entry;
  const char* opt;  // one option away from its default (nullptr: none)
  int val;
  int prev;         // 0 no prev_init, 1 prev_init outside the ring, 2 inside slot 1 of the ring
};

static void* const kDummy = reinterpret_cast<void*>(0x10000);   // a non-null "device" pointer nobody dereferences
static unsigned char* const kStates = reinterpret_cast<unsigned char*>(0x40000000);
// the fields of a table-family source, each its own sentinel
static void* const kRowsF = reinterpret_cast<void*>(0x11000);
static void* const kRowsD = reinterpret_cast<void*>(0x12000);
static void* const kLoads = reinterpret_cast<void*>(0x20000);
static void* const kBnd = reinterpret_cast<void*>(0x30000);
static void* const kKp = reinterpret_cast<void*>(0x50000);
static void* const kNetIdx = reinterpret_cast<void*>(0x60000);
constexpr int kKpK = 3;
constexpr unsigned long long kKpLo = 0x0000000100000005ull, kKpHi = 0x8000000000000002ull;
constexpr int64_t kSteps = 2;

static void set_option(kr_handle& h, const char* opt, int val) {
  const std::string o = opt;
  if (o == "overlap") h.overlap = val;
  else if (o == "msw_overlap") h.msw_overlap = val;
  else if (o == "waves_per_rod") h.waves_per_rod = val;
  else if (o == "persistent") h.persistent = val;
  else if (o == "ms_mode") h.ms_mode = val;
  else if (o == "ms_batch_limit") h.ms_batch_limit = val;
  else if (o == "lds_limit") h.lds_limit = val;
  else if (o == "mfma_mlp") h.mfma_mlp = val;
  else { std::fprintf(stderr, "unknown option %s\n", opt); std::exit(2); }
}

template <typename T>
static void set_net(kr::MlpDev<T>& M, int kind) {
  M = kr::MlpDev<T>{};
  if (kind == 0 || kind == 5) return;
  M.n_layers = 3;
  M.dims[0] = 28; M.dims[1] = 64; M.dims[2] = 64; M.dims[3] = 25;
  M.max_dim = 64;
  M.mfma_ok = kind == 1 || kind == 2 || kind == 4;
  M.jvp_ok = kind == 1 || kind == 4;
}

static void setup_handle(kr_handle& h, const Case& c) {
  h = kr_handle{};
  h.lds_limit = 160 * 1024;
  h.params.N = c.N;
  h.params.nn_input_history = c.net == 4 && c.entry != E_BANK;
  h.cf.N = h.cd.N = c.N;
  h.cf.diag = h.cd.diag = c.diag;
  h.derived.c1 = -40.0; h.derived.c2 = 10.0;
  if (c.entry != E_BANK) { set_net(h.mlp_f, c.net); set_net(h.mlp_d, c.net); }
  h.resume_buf = kDummy;
  h.hist_ws = kDummy;
  h.ws = kDummy;
  if (c.opt) set_option(h, c.opt, c.val);
}

template <typename T>
static kr::SimArgs<T> sim_args(const kr_handle& h, const Case& c) {
  kr::SimArgs<T> a{};
  a.B = c.B; a.T_steps = kSteps;
  a.states = reinterpret_cast<T*>(kStates);
  a.slot_elems = c.B * c.N * KR_SLOTS;
  a.ring = 1;
  a.prev_init = c.prev == 0 ? nullptr : c.prev == 1 ? reinterpret_cast<const T*>(kDummy) : a.states + a.slot_elems + 8;
  a.ctl = static_cast<const T*>(kDummy); a.G = static_cast<T*>(kDummy);
  a.tip = static_cast<T*>(kDummy); a.status = static_cast<int32_t*>(kDummy);
  a.tol = (T)1e-5; a.tolA = (T)3e-3; a.fd_eps = (T)1e-3; a.hc1 = (T)h.derived.c1; a.hc2 = (T)h.derived.c2;
  a.maxit = 30; a.predictor = h.predictor; a.residual_test = h.residual_test;
  a.nn_lowp = h.nn_lowp_first; a.nn_base_only = h.nn_base_only_store;
  return a;
}
template <typename T>
static kr::StepArgs<T> step_args(const kr_handle& h, const Case& c, int mode) {
  kr::StepArgs<T> a{};
  a.B = c.B;
  a.prev = a.cur = static_cast<const T*>(kDummy); a.next = static_cast<T*>(kDummy); a.G = static_cast<T*>(kDummy);
  a.tens = static_cast<const T*>(kDummy); a.tens_stride = 4;
  a.tol = (T)1e-5; a.tolA = (T)3e-3; a.fd_eps = (T)1e-3; a.hc1 = (T)h.derived.c1; a.hc2 = (T)h.derived.c2;
  a.maxit = 30; a.mode = mode; a.st_stride = 1; a.tip_stride = 3; a.residual_test = h.residual_test;
  if (mode == 1) a.r_out = static_cast<T*>(kDummy);
  if (c.entry == E_SIM) {  // step 0 of a simulate call that takes one launch per step
    a.tens_stride = kSteps * 4;
    a.pred = static_cast<double*>(kDummy); a.pred_reset = 1; a.pred_has_prev = c.prev != 0; a.pred_limit = h.predictor;
    a.pred_order = c.prev ? 1 : 0;
  }
  return a;
}

static std::string label(const Case& c) {
  char b[160];
  std::snprintf(b, sizeof b, "%s%s,%d,%lld,%c,d%d,n%d,%s", g_print_src ? "src " : "", c.f64 ? "f64" : "f32", c.N, (long long)c.B,
                c.scheme == KR_EULER ? 'E' : 'R', c.diag, c.net, kEntryName[c.entry]);
  std::string s = b;
  if (c.opt) s += std::string(",") + c.opt + "=" + std::to_string(c.val);
  if (c.prev) s += c.prev == 1 ? ",prev" : ",prev_in_slot1";
  return s;
}

static void print_line(const Case& c, int rc, int path, int overlap, int W) {
  std::string s = label(c) + " | " + std::to_string(rc);
  if (rc == KR_OK) s += " " + std::to_string(path) + " " + std::to_string(overlap) + " " + std::to_string(W);
  else s += " \"" + kr::g_err + "\"";
  s += " |";
  for (size_t i = 0; i < g_launches.size(); ++i) s += (i ? "; " : " ") + g_launches[i];
  std::puts(s.c_str());
}

static void run_case(const Case& c);  // (the interfaces under test)
static void run_pred_matrix();
struct Opt { const char* name; int val; };
// the option values a table-family call refuses or runs under (section 4 of run_matrix and the "src" lines)
static const Opt kTableOpts[] = {{nullptr, 0}, {"ms_mode", 0}, {"ms_mode", 1}, {"persistent", 0}, {"ms_batch_limit", 128}, {"waves_per_rod", 1},
                                 {"waves_per_rod", 2}, {"waves_per_rod", 4}, {"overlap", 0}, {"lds_limit", 65536}, {"mfma_mlp", 0}};

static long run_matrix() {
  long n = 0;
  auto run = [&](const Case& c) {
    g_launches.clear();
    kr::g_err.clear();
    g_attr_kern = nullptr;
    run_case(c);
    ++n;
  };
  const int Ns[] = {8, 9, 31, 32, 40, 55, 56, 100, 128, 129, 400};
  const int64_t Bs[] = {1, 8, 256, 257, 512, 513, 1024, 1025, 2048};
  const int schemes[] = {KR_EULER, KR_RK4};
  // 1. the full product at default options
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : Ns)
      for (int64_t B : Bs)
        for (int scheme : schemes)
          for (int diag = 1; diag >= 0; --diag)
            for (int net = 0; net < 6; ++net)
              for (int entry : {E_SIM, E_STEP, E_RESID})
                run(Case{f64 != 0, N, B, scheme, diag, net, entry, nullptr, 0, 0});
  // 2. one option at a time away from its default
  const Opt opts[] = {{"overlap", 0}, {"msw_overlap", 0}, {"waves_per_rod", 1}, {"waves_per_rod", 2}, {"waves_per_rod", 4},
                      {"persistent", 0}, {"ms_mode", 0}, {"ms_mode", 1}, {"ms_batch_limit", 128}, {"lds_limit", 65536}};
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : {40, 100, 400})
      for (int64_t B : {(int64_t)256, (int64_t)1024})
        for (const Opt& o : opts)
          for (int scheme : schemes)
            for (int diag = 1; diag >= 0; --diag)
              for (int net : {0, 1})
                for (int entry : {E_SIM, E_STEP})
                  run(Case{f64 != 0, N, B, scheme, diag, net, entry, o.name, o.val, 0});
  // (past 1024 rods without the overlapped kernel: the fp32 two-wavefronts-per-SIMD instantiation)
  for (int f64 = 0; f64 < 2; ++f64) run(Case{f64 != 0, 100, 2048, KR_EULER, 1, 0, E_SIM, "overlap", 0, 0});
  // 3. prev_init outside the ring and inside slot 1 of it (the aliasing rule of the overlapped several-wavefront kernel)
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : {100, 400})
      for (int prev : {1, 2})
        run(Case{f64 != 0, N, 512, KR_EULER, 1, 0, E_SIM, nullptr, 0, prev});
  // 4. table and bank entries, with the option values and the scheme they refuse
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : {8, 9, 100, 128, 129})
      for (int64_t B : {(int64_t)8, (int64_t)2048})
        for (int scheme : schemes)
          for (const Opt& o : kTableOpts) {
            for (int net = 0; net < 6; ++net) run(Case{f64 != 0, N, B, scheme, 1, net, E_TAB, o.name, o.val, 0});
            for (int net = 1; net < 4; ++net) run(Case{f64 != 0, N, B, scheme, 1, net, E_BANK, o.name, o.val, 0});
          }
  // 5. kr_simulate_prepare for the headline problem (fp64, and fp32 past 1024 rods): the kernels it readies
  for (int f64 = 0; f64 < 2; ++f64)
    for (int64_t B : {(int64_t)1024, (int64_t)2048})
      run(Case{f64 != 0, 100, B, KR_EULER, 1, 0, E_PREP, nullptr, 0, 0});
  return n;
}

// the matrix of section 4 for all five table-family sources, every line with the source struct the kernel received
static long run_src_matrix() {
  long n = 0;
  g_print_src = true;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : {8, 9, 100, 128, 129})
      for (int64_t B : {(int64_t)8, (int64_t)2048})
        for (int scheme : {KR_EULER, KR_RK4})
          for (const Opt& o : kTableOpts)
            for (int entry : {E_TAB, E_BANK, E_LOADS, E_BND, E_KP})
              for (int net = entry == E_BANK ? 1 : 0; net < (entry == E_BANK ? 4 : 6); ++net, ++n) {
                g_launches.clear();
                kr::g_err.clear();
                g_attr_kern = nullptr;
                run_case(Case{f64 != 0, N, B, scheme, 1, net, entry, o.name, o.val, 0});
              }
  g_print_src = false;
  return n;
}

int main() {
  const long n = run_matrix();
  std::printf("# %ld cases\n", n);
  std::printf("# %ld source cases\n", run_src_matrix());
  run_pred_matrix();
  return 0;
}

// ---- the interfaces under test ----
template <typename T>
static void run_typed(const Case& c) {
  kr_handle h;
  setup_handle(h, c);
  const int use_nn = c.net != 0;
  kr::SimPlan p;
  int rc = KR_OK;
  // (sentinels where the call's writer of last_* has to write; a step call leaves last_overlap, and last_sim_path unless
  // a multiple-shooting kernel took it)
  h.last_waves_per_rod = -1;
  if (c.entry != E_STEP && c.entry != E_RESID) h.last_sim_path = h.last_overlap = -1;
  if (c.entry == E_STEP || c.entry == E_RESID) {
    auto a = step_args<T>(h, c, c.entry == E_RESID ? 1 : 0);
    g_expect = step_scalars(a);
    p = kr::plan_step<T>(&h, c.B, c.scheme, use_nn, a.mode);
    if (!p.rc) rc = kr::launch_step<T>(&h, p, a, nullptr);
    if (!p.rc && !rc) kr::note_step_plan(&h, p);
  } else {
    kr_param_table t;
    t.B = c.B; t.N = c.N;
    t.rows_f = static_cast<kr::RodConst<float>*>(kRowsF); t.rows_d = static_cast<kr::RodConst<double>*>(kRowsD);
    kr_mlp_bank bk;
    bk.K = 3; bk.stride = 256;
    set_net(bk.mf, c.net); set_net(bk.md, c.net);
    kr::SimSrc src;
    switch (c.entry) {
      case E_TAB: src.kind = kr::KR_SRC_TABLE; break;
      case E_BANK: src.kind = kr::KR_SRC_BANK; src.bank = &bk; src.net_idx = static_cast<const int32_t*>(kNetIdx); break;
      case E_LOADS: src.kind = kr::KR_SRC_LOADS; src.hist = kLoads; break;
      case E_BND: src.kind = kr::KR_SRC_BOUNDARY; src.hist = kBnd; break;
      case E_KP: src.kind = kr::KR_SRC_KEYPOINTS; src.hist = kBnd; src.kp = kr::KpDst{kKp, kKpK, kKpLo, kKpHi}; break;
      default: break;  // (the handle's own rod)
    }
    if (src.kind != kr::KR_SRC_HANDLE) src.table = &t;
    auto sa = sim_args<T>(h, c);
    g_expect = sim_scalars(sa);
    p = kr::plan_simulate<T>(&h, kr::plan_query(src, c.B, kSteps, c.scheme, use_nn, sa.prev_init, sa.states, sa.slot_elems));
    if (!p.rc && p.path == 2) {
      rc = kr::launch_sim<T>(&h, p, src, sa, kr::LaunchAt{nullptr, c.entry == E_PREP});
    } else if (!p.rc) {  // step 0 of the per-step loop
      auto a = step_args<T>(h, c, 0);
      g_expect = step_scalars(a);
      rc = kr::launch_step<T>(&h, p, a, nullptr);
    }
    if (!p.rc && !rc && c.entry != E_PREP) kr::note_sim_plan(&h, p, kr::PredImage{}, c.B);
  }
  if (p.rc) { rc = p.rc; kr::g_err = p.why; }
  if (c.entry == E_PREP) print_line(c, rc, p.path, p.overlap, p.W);  // (writes nothing to the handle)
  else print_line(c, rc, h.last_sim_path, h.last_overlap, h.last_waves_per_rod);
}

static void run_case(const Case& c) {
  if (c.f64) run_typed<double>(c);
  else run_typed<float>(c);
}

// ---- the predictor image of a simulate call: plan_pred_image and what note_sim_plan leaves in pred_valid_* ----
static void run_pred_matrix() {
  struct NB { int N; int64_t B; };
  const NB nbs[] = {{100, 256}, {100, 1024}, {400, 1024}, {8, 8}, {8, 100000}};  // (the last: more than 1 GB of images)
  const Opt opts[] = {{nullptr, 0}, {"ms_mode", 0}, {"ms_mode", 1}, {"ms_batch_limit", 128}};
  for (const NB& nb : nbs)
    for (int net : {0, 1})
      for (int persistent : {1, 0})
        for (const Opt& o : opts)
          for (int predictor : {2, 8})
            for (int keep : {0, 1})
              for (int valid = 0; valid < 5; ++valid) {  // image in the buffer: none, this call's, other B, other W, other network state
                const Case c{true, nb.N, nb.B, KR_EULER, 1, net, E_SIM, o.name, o.val, 0};
                kr_handle h;
                setup_handle(h, c);
                h.persistent = persistent; h.predictor = predictor; h.keep_predictor = keep;
                const kr::SimPlan p = kr::plan_simulate<double>(&h, kr::PlanQuery{c.B, kSteps, c.scheme, net});
                if (p.rc) { std::fprintf(stderr, "pred matrix: %s refused\n", label(c).c_str()); std::exit(2); }
                h.pred_valid_B = valid == 0 ? 0 : valid == 2 ? c.B + 1 : c.B;
                h.pred_valid_W = valid == 3 ? (p.W == 1 ? 2 : 1) : p.W;
                h.pred_valid_nn = (p.nn ? 1 : 0) ^ (valid == 4);
                const kr::PredImage im = kr::plan_pred_image(&h, p, c.B);
                kr::note_sim_plan(&h, p, im, c.B);
                std::printf("pred N=%d B=%lld net=%d persistent=%d %s=%d predictor=%d keep=%d valid=%d | %d %d %d | %d %lld %d | %lld %d %d\n",
                            c.N, (long long)c.B, net, persistent, o.name ? o.name : "none", o.val, predictor, keep, valid, p.path, p.W,
                            (int)p.nn, (int)im.use, (long long)im.rows, (int)im.load, (long long)h.pred_valid_B, h.pred_valid_W,
                            h.pred_valid_nn);
              }
}
