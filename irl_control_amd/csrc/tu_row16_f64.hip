// fp64-arithmetic row16 path, double records; row16_tree_masks lives here (see tu_row16_impl.hpp)
#define IRLOSC_R16_TIN double
#define IRLOSC_R16_TREE_MASKS
#include "tu_row16_impl.hpp"
