// Device-only unit of the wave engine, compiled at run time (hiprtc, sf_wave_spec.h) for the constants of one context: exactly one
// k_list_search_wave<SF_SPEC_L, false, 2, true, SF_SPEC_WPE> -- the COMPACT FAST + SMALL kernel of launch modes 3 / 4 / 5 -- with the model's
// constants defined as literals through the SF_SPEC_* macros of sf_list_wave.hip.  No host declaration: nothing of sf_launch.h.
//   -DSF_SPEC_L=2|4      score levels of the instantiation
//   -DSF_SPEC_WPE=4|5|6  waves per SIMD it is compiled for (launch mode 3 / 4 / 5)
//   -DSF_SPEC_V(x)=.. -DSF_SPEC_DIM(x)=.. -DSF_SPEC_NCAP(x)=.. -DSF_SPEC_K0(x)=.. -DSF_SPEC_K1(x)=..
//   -DSF_SPEC_NO_WIDE -DSF_SPEC_NO_TIES -DSF_SPEC_ROWS_FULL -DSF_SPEC_TIE_KEY -DSF_SPEC_RB=.. -DSF_SPEC_PB=..   facts of the neighbour index
//   -DSF_SPEC_SYM_ROWS -DSF_SPEC_LEG_REAIM   the replay batch's leg gathers: source-side rows (a symmetric matrix), discarded gathers re-aimed
#ifndef SF_SPEC_L
#error "SF_SPEC_L: 2 or 4"
#endif
#ifndef SF_SPEC_WPE
#error "SF_SPEC_WPE: 4, 5 or 6"
#endif
#include <hip/hip_runtime.h>

#include "sf_list_model.h"
#include "sf_list_kernels.hip"  // (the helpers the wave engine shares with the block engine; its plain kernels stay uninstantiated templates here)
#include "sf_list_wave.hip"

namespace sf {
template __global__ void k_list_search_wave<SF_SPEC_L, false, 2, true, SF_SPEC_WPE, false>(ListModel m, SearchParams p, NbrIndex nb);
}  // namespace sf
