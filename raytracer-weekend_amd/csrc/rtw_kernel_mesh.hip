// rtw_kernel_mesh.hip — the F_MESHES path-kernel variants (cow, monument, the other triangle worlds) in a
// translation unit of their own, so that the Makefile can build them with the iterative-ILP machine scheduler
// (KFLAGS_MESH) while every other variant keeps max-ILP.  The kernel source is the device headers', the same text
// rtw_kernel.hip compiles; pick_mesh instantiates the mesh variants here, and rtw_kernel.hip's pick_kernel calls it.
#include "rtw_variants.hpp"

namespace rtw {
Variant pick_mesh(const Knobs& kn, uint32_t need, bool half, bool codes16) {
  return pick5<F_MESHES>(kn, need, half, codes16);
}
}  // namespace rtw
