// gg_stats.h — what the statistics trace (gg_stats.hip) sees of the coherent
// mode's state (gg_coherent.hip): the launch state the scan kernel reads.
#pragma once
#include "gg_coh_dev.h"

// The launch state of the context's coherent mode, allocated on first use as
// gg_coherent_begin does (nothing is reset or launched); *begun: a run has
// been begun on it.  The pointers live as long as the context.
gg_status gg_coh_launch_state(gg_ctx* ctx, const ggc::CP** P, const ggc::CS** S, bool* begun);
