// float instantiation of the persistent kernels with per-step boundary data and key-point records (kr_kp_impl.hpp)
#define KR_MS_NO_INST
#include "kr_kp_impl.hpp"
namespace kr {
template int launch_kp_sim<float>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<float>&, const LaunchAt&);
}
