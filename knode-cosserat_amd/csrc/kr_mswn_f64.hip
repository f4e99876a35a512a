// double instantiation of the several-wavefront persistent kernel with the MLP on (kr_mswn_impl.hpp)
#define KR_MS_NO_INST
#include "kr_mswn_impl.hpp"
namespace kr {
template int launch_msw_nn_sim<double>(kr_handle*, const SimPlan&, const SimArgs<double>&, const LaunchAt&);
template int launch_msw_gh_sim<double>(kr_handle*, const SimPlan&, const SimArgs<double>&, const LaunchAt&);
}
