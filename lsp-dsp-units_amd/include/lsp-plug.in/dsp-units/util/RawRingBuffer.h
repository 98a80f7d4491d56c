// lsp::dspu::RawRingBuffer: a plain ring of floats in host memory with its storage in the open.
//
// Binary layout: the reference's three data members in the reference's order (util/RawRingBuffer.h:38-40 of lsp-dsp-units;
// 24 bytes, LP64) and its whole public interface, written from the header's contract.  A host class: nothing of it runs on
// the device.  As Sidechain::sBuffer it carries the capacity and the write position of the sidechain's ring; the samples of
// that ring live on the device (mi_sidechain_bank_*), the storage here stays as init() and fill() left it.
#ifndef MI_LSP_PLUG_IN_DSP_UNITS_UTIL_RAWRINGBUFFER_H_
#define MI_LSP_PLUG_IN_DSP_UNITS_UTIL_RAWRINGBUFFER_H_

#include <lsp-plug.in/dsp-units/version.h>
#include <lsp-plug.in/dsp-units/iface/IStateDumper.h>

namespace lsp
{
    namespace dspu
    {
        class LSP_DSP_UNITS_PUBLIC RawRingBuffer
        {
            protected:
                float      *pData;
                size_t      nCapacity;
                size_t      nHead;

            public:
                explicit RawRingBuffer();
                RawRingBuffer(const RawRingBuffer &) = delete;
                RawRingBuffer(RawRingBuffer &&) = delete;
                ~RawRingBuffer();

                RawRingBuffer & operator = (const RawRingBuffer &) = delete;
                RawRingBuffer & operator = (RawRingBuffer &&) = delete;

                void                construct();            // valid on raw memory
                bool                init(size_t size);      // `size` zeroed samples, the position at 0; what was stored is lost
                void                destroy();

            public:
                // at the head, without moving it: min(count, size()) samples, wrapping at the end; returns what was written
                size_t              write(const float *src, size_t count);
                void                write(float data);
                // the same, and the head moves behind what was written.  As in the reference (RawRingBuffer.cpp:106-125) the block
                // form wraps the position only where it would pass the end: a block that ends AT the ring's end leaves
                // position() == size() and head() == end(), and the next block starts over from begin().  The single-sample
                // forms take such a position as 0 (the reference writes one sample past its storage there)
                size_t              push(const float *data, size_t count);
                void                push(float data);
                // `count` samples from `offset` samples behind the head on (oldest first), wrapping; returns what was read
                size_t              read(float *dst, size_t offset, size_t count);
                float               read(size_t offset) const;
                // the head `count` samples further; returns the new head
                float              *advance(size_t count);

            public:
                inline size_t       size() const                { return nCapacity; }
                void                clear();                // zeroes, the position at 0
                void                reset();                // the position at 0
                inline float       *begin()                     { return pData; }
                inline const float *begin() const               { return pData; }
                inline float       *end()                       { return &pData[nCapacity]; }
                inline const float *end() const                 { return &pData[nCapacity]; }
                inline float       *head()                      { return &pData[nHead]; }
                inline const float *head() const                { return &pData[nHead]; }
                inline size_t       position() const            { return nHead; }
                // the sample `offset` behind the head
                float              *tail(size_t offset);
                const float        *tail(size_t offset) const;
                // samples from the head, from that tail, from whichever is nearer, to the end of the storage
                inline size_t       head_remaining() const      { return nCapacity - nHead; }
                size_t              tail_remaining(size_t offset) const;
                size_t              remaining(size_t offset) const;
                void                fill(float value);      // every sample; the position stays

                void                dump(IStateDumper *v) const;
        };
    }
}

#endif
