// n_links = 1: k_rollout_seq of this link count (fgx_seq_nl.h).
#define FGX_NL 1
#include "fgx_seq_nl.h"
