// double instantiation of the persistent kernel with per-rod networks, per-step boundary data and key-point records (kr_bankkp_impl.hpp)
#define KR_MS_NO_INST
#include "kr_bankkp_impl.hpp"
namespace kr {
template int launch_bankkp_sim<double>(kr_handle*, const SimSrc&, const SimPlan&, const SimArgs<double>&, const LaunchAt&);
}
