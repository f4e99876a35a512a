// float instantiation of the overlapped persistent kernel (kr_mso_impl.hpp)
#define KR_MS_NO_INST
#include "kr_mso_impl.hpp"
namespace kr {
template int launch_mso_sim<float>(kr_handle*, const SimPlan&, const SimArgs<float>&, const LaunchAt&);
}
