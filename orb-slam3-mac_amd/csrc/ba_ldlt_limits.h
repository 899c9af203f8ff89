// ba_ldlt_limits.h -- the largest system of the single-workgroup dense LDL^T (ba_ldlt.h).  Nothing from HIP is included: the host-only
// list builders (ba_graph_lists.h, iba_pack.h) refuse or reroute larger systems by the same number the kernels are sized with.
#pragma once
#define BA_LDLT_MAXN 480
