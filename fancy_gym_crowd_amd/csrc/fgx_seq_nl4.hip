// n_links = 4: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 4
#include "fgx_seq_nl.h"
