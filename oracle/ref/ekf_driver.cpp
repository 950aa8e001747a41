// Driver of the firmware's own EKF (ekf.cpp, compiled unmodified by oracle/ref/Makefile).  TEST INFRASTRUCTURE ONLY.
//
// stdin: one operation per line, numbers as C99 hexadecimal floats (strtod reads them back exactly):
//   I t x0 x1 x2 x3 x4 x5      a new EKF object, then EKF::init(t, x0): init alone keeps the covariance, and the firmware calls
//                              it once per object
//   P omega t                  EKF::predict(imu with angular_velocity.z = omega, t)
//   U z_v z_omega              EKF::update(odometry with twist.linear.x = z_v, twist.angular.z = z_omega)
//   N                          a new EKF object, not initialised (the next stream)
// stdout: after every I, P and U, 42 raw doubles: x[6], then P[36] row-major.
// The covariance is private in ekf.h; the Makefile opens it with -Dprivate=public on both translation units.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ekf.h"

static void emit(const EKF &f)
{
    double out[42];
    for (int i = 0; i < 6; i++) out[i] = f.x_(i);
    for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) out[6 + 6 * r + c] = f.P_(r, c);
    if (fwrite(out, sizeof(double), 42, stdout) != 42) exit(3);
}

int main()
{
    EKF *f = new EKF();
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        double v[7];
        int n = 0;
        char *p = line + 1;
        while (n < 7) {
            char *end;
            const double d = strtod(p, &end);
            if (end == p) break;
            v[n++] = d; p = end;
        }
        if (line[0] == 'N' && n == 0) { delete f; f = new EKF(); continue; }
        if (line[0] == 'I' && n == 7) {
            Eigen::VectorXd x0(6);
            for (int i = 0; i < 6; i++) x0(i) = v[1 + i];
            delete f; f = new EKF();
            f->init(v[0], x0);
        } else if (line[0] == 'P' && n == 2) {
            sensor_msgs__msg__Imu imu;
            memset(&imu.orientation, 0, sizeof imu.orientation);
            imu.angular_velocity.x = imu.angular_velocity.y = 0.0;
            imu.linear_acceleration.x = imu.linear_acceleration.y = imu.linear_acceleration.z = 0.0;
            imu.angular_velocity.z = v[0];
            f->predict(imu, v[1]);
        } else if (line[0] == 'U' && n == 2) {
            nav_msgs__msg__Odometry od;
            od.twist.twist.linear.x = v[0];
            od.twist.twist.angular.z = v[1];
            f->update(od);
        } else {
            fprintf(stderr, "ekf_driver: bad line: %s", line);
            return 2;
        }
        emit(*f);
    }
    delete f;
    return 0;
}
