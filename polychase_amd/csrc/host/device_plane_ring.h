// device_plane_ring.h -- a few device planes of one size, owned by one analysis run: the mesh masks of the frames being put
// (analysis_driver.cc renders a frame's mask into a plane, hands it to pc_analyzer_set_mask(on_device = 1) and must keep it
// alive and unmodified until pc_analyzer_frame_ingested says so for the frame put under it).  A plane is taken together with
// a token; it is free again when the last copy of the token is gone -- the driver parks the token next to the frame's own
// owner, so the rule that releases ingested frames releases the plane.  Planes are allocated by the first Take and freed by
// the destructor, which therefore has to run after the last reader is done (declare the ring in front of whatever holds
// tokens and in front of the engine).  Not thread safe: one run, one thread.  No GPU call of its own: allocation and release
// are the caller's functions, so the lifetime logic runs in a plain C++ program (tools/sanitize/device_plane_ring_check.cc).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <utility>
#include <vector>

class DevicePlaneRing {
   public:
    using Alloc = std::function<void*(size_t bytes)>;   // throws, or returns a plane
    using Free = std::function<void(void* plane)>;

    DevicePlaneRing(int slots, size_t plane_bytes, Alloc alloc, Free release)
        : slots_(static_cast<size_t>(slots > 0 ? slots : 1)), bytes_(plane_bytes), alloc_(std::move(alloc)), free_(std::move(release)) {}
    DevicePlaneRing(const DevicePlaneRing&) = delete;
    DevicePlaneRing& operator=(const DevicePlaneRing&) = delete;
    ~DevicePlaneRing() {
        for (Slot& s : slots_)
            if (s.plane) free_(s.plane);
    }

    // A free plane and its token, or {nullptr, nullptr} while every plane is taken (the caller lets go of tokens and asks again).
    std::pair<uint8_t*, std::shared_ptr<void>> Take() {
        if (!allocated_) {
            for (Slot& s : slots_)
                if (!s.plane) s.plane = alloc_(bytes_);   // an exception leaves what exists to the destructor (and to the next Take)
            allocated_ = true;
        }
        for (size_t k = 0; k < slots_.size(); k++) {
            Slot& s = slots_[(next_ + k) % slots_.size()];
            if (s.taken) continue;
            next_ = (next_ + k + 1) % slots_.size();
            s.taken = true;
            return {static_cast<uint8_t*>(s.plane), std::shared_ptr<void>(&s, [](void* p) { static_cast<Slot*>(p)->taken = false; })};
        }
        return {nullptr, nullptr};
    }
    int Taken() const {
        int n = 0;
        for (const Slot& s : slots_) n += s.taken ? 1 : 0;
        return n;
    }
    size_t size() const { return slots_.size(); }

   private:
    struct Slot {
        void* plane = nullptr;
        bool taken = false;
    };
    std::vector<Slot> slots_;   // never resized: tokens point into it
    size_t bytes_;
    Alloc alloc_;
    Free free_;
    bool allocated_ = false;
    size_t next_ = 0;
};
