// The translation unit of the scalar construction phase: k_scalar_construct (sf_scalar_construct.hip), built once with the general scalar
// configuration -- the interpreted pair-predicate joins in, both the class's own join and the loop over the join records of a multi-join
// class (SF_SCALAR_PAIR_IR 1, SF_SCALAR_MULTI_JOIN 1: what the plain kernels of the C-ABI unit are built with) -- so that one kernel
// prices every constraint form.  The plain kernels themselves are uninstantiated templates here (SF_TU_MAIN is not defined).
#define SF_TU_ENGINES 7
#include "sf_launch.h"
#include "sf_scalar_construct.hip"
