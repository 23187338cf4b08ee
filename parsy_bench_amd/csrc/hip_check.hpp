// The one HIP error check of the host side of the .hip translation units: a failing call leaves
// "<call text>: <hipGetErrorString>" as the thread's last error and makes the enclosing function return.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "errors.hpp"

#define PARSY_HIP_OR(call, ret)                                                               \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            ::parsy::set_last_error(std::string(#call) + ": " + hipGetErrorString(e_));       \
            return ret;                                                                       \
        }                                                                                     \
    } while (0)
#define PARSY_HIP(call) PARSY_HIP_OR(call, -1)
