// n_links = 5: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 5
#include "fgx_seq_nl.h"
