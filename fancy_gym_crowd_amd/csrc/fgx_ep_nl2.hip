// n_links = 2: every kernel family of this link count (fgx_ep_nl.h).
#define FGX_NL 2
#include "fgx_ep_nl.h"
