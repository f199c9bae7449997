/* msd_devbuf.h -- an owning, grow-only array in device memory: a pointer and how many elements it has room for.  What
 * msd_pos.cpp keeps its buffers in, so that a buffer is named where it is declared and where it is used, and nowhere
 * to be freed.  Host code only: plain C++17 against the HIP runtime headers. */
#ifndef MSD_DEVBUF_H
#define MSD_DEVBUF_H

#include <stddef.h>

#include <hip/hip_runtime_api.h>

template <typename T> class msd_devbuf {
  public:
    msd_devbuf() = default;
    msd_devbuf(msd_devbuf &&o) noexcept : ptr_(o.ptr_), cap_(o.cap_) { o.ptr_ = nullptr, o.cap_ = 0; }
    msd_devbuf &operator=(msd_devbuf &&o) noexcept
    {
        if (this != &o) {
            drop();
            ptr_ = o.ptr_, cap_ = o.cap_;
            o.ptr_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~msd_devbuf() { drop(); }

    /* Room for n elements.  Enough already: nothing happens.  Otherwise what there is goes first and exactly n elements
     * are allocated -- nothing on top, nothing kept.  After a failure the array is empty, so the next call tries again. */
    hipError_t reserve(size_t n)
    {
        if (n <= cap_)
            return hipSuccess;
        drop();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr_), n * sizeof(T));
        if (e != hipSuccess) {
            ptr_ = nullptr;
            return e;
        }
        cap_ = n;
        return hipSuccess;
    }

    T *get() const { return ptr_; }

  private:
    void drop()
    {
        if (ptr_)
            (void)hipFree(ptr_);
        ptr_ = nullptr, cap_ = 0;
    }

    T *ptr_ = nullptr;
    size_t cap_ = 0;
};

#endif
