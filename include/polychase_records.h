// polychase_records.h -- where the parts of one analyzer job's packed records lie (C++ only, header-only; the format itself is
// documented at pc_analyzer_set_device_log in polychase_hip.h).  The ONE statement of the layout in C++: the analyzer writes by it
// (csrc/hip/api_analyzer.hip), the record writer reads by it (csrc/host/analysis_driver.cc).  polychase_amd/distributed.py
// (record_layout) is its twin in Python, tests/test_distributed_cpu.py holds both to a restatement of its own.
#pragma once

#include <cstddef>

namespace pc {

// A pack: row offsets | keypoints | src indices | tgt xy | errors, every part 16-byte aligned.  A device-log record is a header
// of kLogHeaderBytes followed by the pack.  Offsets count from the start of the pack.
struct RecordLayout {
    static constexpr size_t kLogHeaderBytes = 128;   // int64 hdr[16]: magic, frame1, keypoints, targets, target ids [8], rows
    static constexpr size_t kRowOffsetBytes = 128;   // int64 row_offset[16], written by the GPU
    size_t o_kps = 0, o_idx = 0, o_xy = 0, o_err = 0, bytes = 0;
    RecordLayout() = default;
    RecordLayout(size_t n_keypoints, size_t rows) {   // rows: n_keypoints * n_targets, the capacity of the three row arrays
        auto up16 = [](size_t v) { return (v + 15) & ~static_cast<size_t>(15); };
        o_kps = kRowOffsetBytes;
        o_idx = up16(o_kps + n_keypoints * 8);
        o_xy = up16(o_idx + rows * 4);
        o_err = up16(o_xy + rows * 8);
        bytes = up16(o_err + rows * 4);
    }
};

}  // namespace pc
