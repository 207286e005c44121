// srt_host_internal.h -- what the host mirror's translation units share among themselves (srt_host.cpp, srt_host_render.cpp,
// srt_host_c.cpp).  Not installed and not included by srt_host.h.
#pragma once
#include <cstddef>
#include <cstring>
#include <functional>

#include "srt_host.h"

namespace srt_host {

// fn(begin, end) over [0, n) in chunks of at least `grain`, on the build pool plus the calling thread (srt_host.cpp)
void parallel_for(size_t n, size_t grain, const std::function<void(size_t, size_t)>& fn);

// mat4 <-> 16 floats, column-major (glm::mat4 memory order: m[c][r] at 4 * c + r)
inline mat4 mat4_from_floats(const float* m) { mat4 M; std::memcpy(&M[0][0], m, 64); return M; }
inline void mat4_to_floats(const mat4& M, float* m) { std::memcpy(m, &M[0][0], 64); }

// the light position as callers of the C handles pass it
inline vec4 light_vec4(const float* l) { return vec4(l[0], l[1], l[2], l[3]); }

} // namespace srt_host
