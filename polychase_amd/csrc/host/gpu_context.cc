#include "gpu_context.h"

#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <string>

namespace {
std::mutex g_mtx;
pc_context* g_ctx = nullptr;
int g_device = -1;

int DeviceFromEnvironment() {
    const char* env = std::getenv("POLYCHASE_DEVICE");
    return env ? std::atoi(env) : 0;
}
}  // namespace

pc_context* SharedGpuContext() {
    std::lock_guard<std::mutex> lk(g_mtx);
    if (!g_ctx) {
        const int device = DeviceFromEnvironment();
        if (pc_context_create(device, &g_ctx) != PC_OK)
            throw std::runtime_error(std::string("pc_context_create: ") + pc_last_error());
        g_device = device;
    }
    return g_ctx;
}

int SharedGpuDevice() {
    std::lock_guard<std::mutex> lk(g_mtx);
    return g_ctx ? g_device : DeviceFromEnvironment();
}

std::recursive_mutex& SharedGpuMutex() {
    static std::recursive_mutex mtx;
    return mtx;
}
