// Stand-in for the micro-ROS message header of the ESP32 build: the firmware's own ros_compat.h (on the include path)
// declares nav_msgs__msg__Odometry.
#include "ros_compat.h"
