// The script interface of the streaming drivers (every *_main.cpp that includes this file; stream_rt.cpp holds the
// runtime).  A driver is run as  <driver> in.bin out.bin  and only maps a call's numbers and buffers onto an entry point's
// arguments; the test that wrote in.bin owns every layout.  All integers in both files are int64.
//   in.bin  = nbuf, then per buffer: bytes, off, and the block's `bytes` bytes.  The block is a 16-byte-aligned heap allocation
//             of exactly `bytes` bytes, so an access outside it is the sanitizer's to report; the entry point gets block + off
//             (a channel slice that starts behind poison the test checks afterwards).
//             ncall, then per call: fn, ni, ni integers, nd, nd doubles, nb, nb buffer indices (-1: a null pointer)
//   out.bin = the ncall return values, then every block again, whole
#pragma once
#include <cstdint>
#include <vector>

struct emu_call {
    int fn;
    std::vector<int64_t> i;
    std::vector<double> d;
    std::vector<int64_t> b;
    std::vector<char*> ptr;   // ptr[k]: block b[k] + its off, or null
    template <class T>
    T* p(int k) const { return reinterpret_cast<T*>(ptr[k]); }
    float* f(int k) const { return p<float>(k); }
    int I(int k) const { return (int)i[k]; }
};

// reads the script, runs `dispatch` on every call in order and writes out.bin; the value of main()
int emu_run_script(int argc, char** argv, int64_t (*dispatch)(const emu_call&));

// joins the lane threads emu_launch keeps between launches; a driver with a main() of its own calls it before it returns
void emu_shutdown();
