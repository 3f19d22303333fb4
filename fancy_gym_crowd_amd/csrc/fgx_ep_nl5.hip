// n_links = 5: every kernel family of this link count (fgx_ep_nl.h).
#define FGX_NL 5
#include "fgx_ep_nl.h"
