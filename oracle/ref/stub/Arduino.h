// Stand-in for the Arduino core header the firmware's ekf.h includes: ekf.cpp uses nothing of it beyond <cmath>'s M_PI.
#ifndef QS_REF_ARDUINO_STANDIN_H
#define QS_REF_ARDUINO_STANDIN_H
#include <cmath>
#include <cstdint>
#endif
