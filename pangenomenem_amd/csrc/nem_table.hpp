// nem_table.hpp -- what the C entry points of the two device tables share (nem_matrix.hip: nemgpu_family_table_*,
// nem_edges.hip: nemgpu_edge_table_*): a text call's checks and its text buffer, kept between calls, a device error as a status.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

#include "nem_internal.hpp"
#include "nem_master.hpp"

namespace nemk {

// a batch's text on the device, kept for the next call; the table's handle frees it
struct TableText {
    char* text = nullptr;
    size_t text_cap = 0;
};

// the caller's buffer against the batch's size (*needed, may be null, is told it either way), then room for the batch in t
inline int text_room(const std::string& who, TableText* t, long long capacity, long long bytes, int64_t* needed)
{
    if (needed) *needed = bytes;
    if (capacity < bytes) {
        set_error(who + ": the buffer holds " + std::to_string(capacity) + " bytes, the batch needs " + std::to_string(bytes));
        return NEMGPU_E_ARG;
    }
    if (t->text_cap >= (size_t)bytes) return NEMGPU_OK;
    if (t->text) (void)hipFree(t->text);
    t->text = nullptr; t->text_cap = 0;
    HIPCHK(hipMalloc((void**)&t->text, a256((size_t)bytes)));
    t->text_cap = a256((size_t)bytes);
    return NEMGPU_OK;
}

// a text call's master and rows against the table's n, d, device and its `count` rows
inline int check_batch(const std::string& who, const nemgpu_master* m, int n, int d, int device, int row0, int rows, int count)
{
    if (m->n != n || m->d != d || m->device != device) { set_error(who + ": not the table's master"); return NEMGPU_E_ARG; }
    if (row0 < 0 || rows <= 0 || (long long)row0 + rows > count) { set_error(who + ": rows outside the table"); return NEMGPU_E_ARG; }
    return NEMGPU_OK;
}

// what a call's launches, copies and its wait came to, as the entry point's status
inline int device_status(const std::string& who, hipError_t err)
{
    if (err == hipSuccess) return NEMGPU_OK;
    (void)hipGetLastError();
    set_error(who + ": " + hipGetErrorString(err));
    return NEMGPU_E_DEVICE;
}

}  // namespace nemk
