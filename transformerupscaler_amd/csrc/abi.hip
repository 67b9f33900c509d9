#include "tupscale_hip.h"
extern "C" int tup_abi_version(void) { return TUP_ABI_VERSION; }
