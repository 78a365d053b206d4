// device_plane_ring_check.cc -- the lifetime logic of csrc/host/device_plane_ring.h in a plain program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I polychase_amd/csrc/host tools/sanitize/device_plane_ring_check.cc -o /tmp/ring_check && /tmp/ring_check
// Planes are heap blocks here; the "analyzer" is a queue of frames that become ingested a few puts later, as in the driver.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <set>

#include "device_plane_ring.h"

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main() {
    std::set<void*> live;
    size_t allocs = 0;
    {
        DevicePlaneRing ring(
            4, 1000,
            [&](size_t bytes) {
                void* p = std::malloc(bytes);
                live.insert(p);
                allocs++;
                return p;
            },
            [&](void* p) {
                REQUIRE(live.erase(p) == 1);
                std::free(p);
            });
        REQUIRE(allocs == 0 && ring.Taken() == 0);   // nothing until the first Take
        std::deque<std::pair<int, std::shared_ptr<void>>> in_flight;   // declared behind the ring: let go of first
        std::shared_ptr<void> fixed;
        {
            auto t = ring.Take();
            REQUIRE(t.first && allocs == 4);
            std::memset(t.first, 0xff, 1000);
            fixed = t.second;
        }
        REQUIRE(ring.Taken() == 1);
        std::set<uint8_t*> busy;
        for (int frame = 0; frame < 100; frame++) {
            auto t = ring.Take();
            while (!t.first) {   // every plane waits for a frame: the oldest is ingested
                REQUIRE(!in_flight.empty());
                in_flight.pop_front();
                t = ring.Take();
            }
            std::memset(t.first, frame, 1000);
            in_flight.emplace_back(frame, t.second);
            in_flight.emplace_back(frame, fixed);          // the fixed token may wait with many frames
            REQUIRE(ring.Taken() <= 4 && allocs == 4);
            busy.clear();
            for (auto& f : in_flight) busy.insert(static_cast<uint8_t*>(f.second.get()));
            REQUIRE((int)busy.size() == ring.Taken());    // a plane is taken exactly while a token of it exists
            if (frame % 3 == 0 && !in_flight.empty()) in_flight.pop_front();
        }
        in_flight.clear();
        REQUIRE(ring.Taken() == 1);
        fixed.reset();
        REQUIRE(ring.Taken() == 0);
        // an allocation that throws half way leaves the planes made so far to the destructor
        int n = 0;
        DevicePlaneRing broken(
            3, 10,
            [&](size_t bytes) -> void* {
                if (++n == 3) throw std::runtime_error("out of memory");
                void* p = std::malloc(bytes);
                live.insert(p);
                return p;
            },
            [&](void* p) {
                REQUIRE(live.erase(p) == 1);
                std::free(p);
            });
        bool threw = false;
        try {
            broken.Take();
        } catch (const std::runtime_error&) {
            threw = true;
        }
        REQUIRE(threw && live.size() == 6);
    }
    REQUIRE(live.empty());
    std::puts("device_plane_ring_check: ok");
    return 0;
}
