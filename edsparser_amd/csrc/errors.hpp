// errors.hpp — what the library throws, without a HIP include: the C ABI maps each type to a status (capi.hip).
#pragma once

#include <stdexcept>

namespace edsx {

struct FormatError : std::runtime_error { using std::runtime_error::runtime_error; };   // EDSX_ERR_INVALID_FORMAT
struct ParamError : std::runtime_error { using std::runtime_error::runtime_error; };    // EDSX_ERR_INVALID_PARAMETER
// a well-formed input beyond a limit of this build (more than MsaPipeline::MAX_ROWS sequences): EDSX_ERR_BUILD_FAILED,
// not a format error - the reference has no such limit
struct LimitError : std::runtime_error { using std::runtime_error::runtime_error; };
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };

} // namespace edsx
