// float instantiation of the persistent kernel with per-rod parameter tables and per-rod networks (kr_bank_impl.hpp)
#define KR_MS_NO_INST
#include "kr_bank_impl.hpp"
namespace kr {
template int launch_bank_sim<float>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<float>&, const LaunchAt&);
}
