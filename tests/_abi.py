"""The C ABI number as the tests expect it: a literal of their own, deliberately not read from the binding or from
include/tupscale_hip.h (TUP_ABI_VERSION), so that a bump edits that define and this line and every per-feature test then
checks the two against each other and against the built library."""
ABI = 16          # 16: seven entries removed, none changed
