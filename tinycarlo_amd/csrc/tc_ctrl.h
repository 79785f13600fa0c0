// Built-in controllers of the simulate kernels (tc_env_set_controller): the action of a step computed on the device from
// what the env reported after its previous step, so that a closed control loop runs inside one K-step launch.
//
// Stanley lateral controller of the reference's examples/stanley_control.py:56-57 and of the data collection of
// examples/train_stanley_il.py:
//   steering_correction = math.atan2(k * cte, speed)
//   steering_angle = (heading_error + steering_correction) * 180 / math.pi / config["car"]["max_steering_angle"]
// evaluated left to right like the Python expression, every operation rounded on its own (the library is built with
// -ffp-contract=off), atan2 being tc_atan2 (tc_trig.h) like every other atan2 of the library.
// Plain C / HIP like tc_trig.h and tc_rng.h: the tests build this header with the host compiler.
#ifndef TC_CTRL_H
#define TC_CTRL_H
#include "tc_trig.h" /* TC_HD, tc_atan2 */

TC_HD double tc_ctrl_stanley(double cte, double he, double k, double speed, double max_steering_angle_deg) {
  return (((he + tc_atan2(k * cte, speed)) * 180.0) / 3.141592653589793) / max_steering_angle_deg;
}

#endif  // TC_CTRL_H
