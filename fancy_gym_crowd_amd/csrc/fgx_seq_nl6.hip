// n_links = 6: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 6
#include "fgx_seq_nl.h"
