// Module k8s_amd._C: every kernel family's entry points (one bind_<family> per file of this directory) and the
// module-level constants.
#include "binding/common.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  using namespace k8s_amd::binding;
  m.doc() = "k8s_amd gfx950 (MI355X) HIP kernels";
  for (auto bind : {bind_optim, bind_batchnorm, bind_norm, bind_gemm, bind_conv, bind_attention, bind_elementwise,
                    bind_data, bind_decode})
    bind(m);
  m.def("planner_cus", &k8s_amd::planner_cus,
        "CUs the launch planners size grids for (the device's multiprocessor count unless overridden)");
  m.def("set_planner_cus", &k8s_amd::set_planner_cus, "n"_a,
        "override the planners' CU budget for every device (n <= 0: back to the device's count)");
  m.attr("arch") = "gfx950";
  m.attr("conv_stat_replicas") = k8s_amd::kConvStatReplicas;
  m.attr("layer_item_max") = k8s_amd::kLayerItemMax;
}
