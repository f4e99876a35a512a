// double instantiation of the persistent kernels with per-rod parameter tables and per-step tip loads (kr_load_impl.hpp)
#define KR_MS_NO_INST
#include "kr_load_impl.hpp"
namespace kr {
template int launch_load_sim<double>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<double>&, const LaunchAt&);
}
