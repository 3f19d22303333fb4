// n_links = 7: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 7
#include "fgx_seq_nl.h"
