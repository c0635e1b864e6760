// Recording stand-in for the HIP runtime symbols libstzs_hip's objects reference (tools/dispatch_trace.py links it
// with styletts-zs_amd/build/*.o into libstzs_trace.so).  Nothing runs on a device and no pointer argument is ever
// dereferenced: a launch is one line "L <kernel> <gx> <gy> <gz> <bx> <by> <bz> <lds>", a hipFuncSetAttribute one line
// "A <kernel> <attribute> <value>", a driver's marker one line "M <text>", appended to the file $HIP_RECORD_OUT names
// (nothing is written without it).  The device answers as an MI355X: 256 CUs, gcnArchName "gfx950".
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

namespace {
std::map<const void*, std::string>& names() {  // host stub -> kernel name (from __hipRegisterFunction)
    static std::map<const void*, std::string> m;
    return m;
}
FILE* out() {
    static FILE* f = [] {
        const char* p = getenv("HIP_RECORD_OUT");
        return p && *p ? fopen(p, "a") : nullptr;
    }();
    return f;
}
const char* name_of(const void* fn) {
    auto it = names().find(fn);
    return it == names().end() ? "?" : it->second.c_str();
}
struct Config { dim3 grid, block; size_t lds; hipStream_t stream; };
thread_local Config g_cfg;
}  // namespace

extern "C" {
void hip_record_mark(const char* text) {
    if (out()) fprintf(out(), "M %s\n", text), fflush(out());
}
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, uint3*, uint3*, dim3*,
                           dim3*, int*) {
    names()[host_fn] = device_name;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    g_cfg = {grid, block, lds, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    *grid = g_cfg.grid, *block = g_cfg.block, *lds = g_cfg.lds, *stream = g_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 g, dim3 b, void**, size_t lds, hipStream_t) {
    if (out())
        fprintf(out(), "L %s %u %u %u %u %u %u %zu\n", name_of(fn), g.x, g.y, g.z, b.x, b.y, b.z, lds), fflush(out());
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
    if (out()) fprintf(out(), "A %s %d %d\n", name_of(fn), (int)attr, value), fflush(out());
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t attr, int) {
    *v = attr == hipDeviceAttributeMultiprocessorCount ? 256 : 0;
    return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
    memset(p, 0, sizeof(*p));
    strcpy(p->gcnArchName, "gfx950");
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void*, const void*, size_t n, hipMemcpyKind, hipStream_t) {
    if (out()) fprintf(out(), "C memcpy %zu\n", n), fflush(out());
    return hipSuccess;
}
hipError_t hipMemsetAsync(void*, int, size_t n, hipStream_t) {
    if (out()) fprintf(out(), "C memset %zu\n", n), fflush(out());
    return hipSuccess;
}
}
