// n_links = 2: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 2
#include "fgx_seq_nl.h"
