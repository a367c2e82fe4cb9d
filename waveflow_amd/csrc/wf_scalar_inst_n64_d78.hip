// explicit instantiations of the scalar kernels (wf_scalar_impl.h): compiled as a separate translation unit
#include "wf_scalar_impl.h"

namespace wf {
namespace scalar {
WF_SCALAR_SHAPE(, 7, 64)
WF_SCALAR_SHAPE(, 8, 64)
}  // namespace scalar
}  // namespace wf
