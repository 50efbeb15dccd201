// scan_ordered.hip — the ordered variants (ScanRequest::ordered) of the
// one-shot scan kernels and their launchers (scan_ordered.hpp). The kernels
// are the templates of scan_kernels.hip, instantiated here with ORD = true
// and nowhere else; scan_kernels.hip instantiates ORD = false only. Why two
// translation units: scan_ordered.hpp.

#define SBG_ORDERED_TU 1
#include "scan_kernels.hip"
