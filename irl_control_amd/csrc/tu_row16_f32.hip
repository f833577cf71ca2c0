// fp64-arithmetic row16 path, float records (see tu_row16_impl.hpp)
#define IRLOSC_R16_TIN float
#include "tu_row16_impl.hpp"
