// n_links = 8: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 8
#include "fgx_seq_nl.h"
