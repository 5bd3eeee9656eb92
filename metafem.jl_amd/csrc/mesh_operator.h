// The matrix-free mesh operator as the solve driver (krylov.hip) and the product dispatch (spmv.hip) see it: through the interface of operator.h
// (mfem_mesh_operator_interface()).  The handle, the kernels and their launches live in mesh_operator.hip, the host decisions in
// mesh_operator_decide.h.
#pragma once
#include "operator.h"
