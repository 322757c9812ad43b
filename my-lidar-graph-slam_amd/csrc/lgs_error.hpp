// lgs_error.hpp -- the library's exception and its argument check, free of the
// HIP runtime so that plain host programs can include them (LGS_HIP_CHECK, which
// needs the runtime, is in lgs_internal.hpp).
#pragma once

#include <stdexcept>
#include <string>

#include "lgs_hip.h"

namespace lgs {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace lgs

#define LGS_REQUIRE(cond, msg)                                                           \
    do {                                                                                 \
        if (!(cond))                                                                     \
            throw ::lgs::Error(LGS_ERR_INVALID_ARG, msg);                                \
    } while (0)
