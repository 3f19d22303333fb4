// n_links = 3: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 3
#include "fgx_seq_nl.h"
