// t2d_math_probe_table.hip -- the T2D_TRIG_TABLE variant of the t2d_debug_math probe: t2d_math_probe.hip compiled once more
// with t2d_math.h reading its polynomial constants from the __constant__ tables, as t2d_collide.hip -- the only product
// translation unit that defines the macro -- compiles it.  tests/test_gpu_math.py holds it bit for bit against the literals.
#define T2D_TRIG_TABLE
#define T2D_MATH_PROBE_TABLE
#include "t2d_math_probe.hip"
