// float instantiation of the persistent kernels with per-rod parameter tables and per-step boundary data (kr_bnd_impl.hpp)
#define KR_MS_NO_INST
#include "kr_bnd_impl.hpp"
namespace kr {
template int launch_bnd_sim<float>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<float>&, const LaunchAt&);
}
