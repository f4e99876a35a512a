// float instantiation of the persistent kernels with per-rod parameter tables (kr_tab_impl.hpp)
#define KR_MS_NO_INST
#include "kr_tab_impl.hpp"
namespace kr {
template int launch_tab_sim<float>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<float>&, const LaunchAt&);
template int launch_tab_init_straight<float>(kr_handle*, const kr_param_table*, float*, hipStream_t);
}
