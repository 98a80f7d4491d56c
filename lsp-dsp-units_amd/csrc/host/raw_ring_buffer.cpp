// lsp::dspu::RawRingBuffer (util/RawRingBuffer.h): a ring of floats in host memory, written from the header's contract.
#include <lsp-plug.in/dsp-units/util/RawRingBuffer.h>

#include <cstdlib>
#include <cstring>

namespace lsp
{
namespace dspu
{
namespace
{
    // the index `offset` samples behind `head` in a ring of `cap`
    inline size_t behind(size_t head, size_t cap, size_t offset) { return (head + cap - offset % cap) % cap; }
}

static_assert(sizeof(void *) != 8 || sizeof(RawRingBuffer) == 24, "the reference's layout: a pointer and two size_t");

RawRingBuffer::RawRingBuffer()  { construct(); }
RawRingBuffer::~RawRingBuffer() { destroy(); }

void RawRingBuffer::construct()
{
    pData = NULL;
    nCapacity = 0;
    nHead = 0;
}

bool RawRingBuffer::init(size_t size)
{
    float *p = static_cast<float *>(realloc(pData, size * sizeof(float)));
    if (p == NULL)
        return false;
    memset(p, 0, size * sizeof(float));
    pData = p;
    nCapacity = size;
    nHead = 0;
    return true;
}

void RawRingBuffer::destroy()
{
    free(pData);
    construct();
}

void RawRingBuffer::clear()
{
    nHead = 0;
    if (pData != NULL)
        memset(pData, 0, nCapacity * sizeof(float));
}

void RawRingBuffer::reset()
{
    nHead = 0;
}

size_t RawRingBuffer::write(const float *src, size_t count)
{
    count = (count < nCapacity) ? count : nCapacity;
    if (count == 0)
        return 0;
    const size_t first = (count < nCapacity - nHead) ? count : nCapacity - nHead;
    memcpy(pData + nHead, src, first * sizeof(float));
    memcpy(pData, src + first, (count - first) * sizeof(float));
    return count;
}

void RawRingBuffer::write(float data)
{
    pData[(nHead < nCapacity) ? nHead : 0] = data;              // see push(float)
}

size_t RawRingBuffer::push(const float *data, size_t count)
{
    count = write(data, count);
    // RawRingBuffer.cpp:110-122: the position wraps only where nHead + count > nCapacity, so a block that ends at the ring's end
    // leaves it AT the capacity (head() == end()), and the next block starts over from there
    nHead = (nHead + count > nCapacity) ? nHead + count - nCapacity : nHead + count;
    return count;
}

void RawRingBuffer::push(float data)
{
    // a position at the capacity (see above) is the ring's start: the reference writes pData[nCapacity] there (:127-131)
    if (nHead >= nCapacity)
        nHead = 0;
    pData[nHead] = data;
    nHead = (nHead + 1) % nCapacity;
}

size_t RawRingBuffer::read(float *dst, size_t offset, size_t count)
{
    if (nCapacity == 0)
        return 0;
    count = (count < nCapacity) ? count : nCapacity;
    const size_t from = behind(nHead, nCapacity, offset);
    const size_t first = (count < nCapacity - from) ? count : nCapacity - from;
    memcpy(dst, pData + from, first * sizeof(float));
    memcpy(dst + first, pData, (count - first) * sizeof(float));
    return count;
}

float RawRingBuffer::read(size_t offset) const
{
    return pData[behind(nHead, nCapacity, offset)];
}

float *RawRingBuffer::advance(size_t count)
{
    nHead = (nHead + count) % nCapacity;
    return &pData[nHead];
}

float *RawRingBuffer::tail(size_t offset)
{
    return &pData[behind(nHead, nCapacity, offset)];
}

const float *RawRingBuffer::tail(size_t offset) const
{
    return &pData[behind(nHead, nCapacity, offset)];
}

size_t RawRingBuffer::tail_remaining(size_t offset) const
{
    return nCapacity - behind(nHead, nCapacity, offset);
}

size_t RawRingBuffer::remaining(size_t offset) const
{
    const size_t t = tail_remaining(offset), h = head_remaining();
    return (t < h) ? t : h;
}

void RawRingBuffer::fill(float value)
{
    for (size_t i = 0; i < nCapacity; ++i)
        pData[i] = value;
}

void RawRingBuffer::dump(IStateDumper *v) const
{
    v->write("pData", pData);
    v->write("nCapacity", nCapacity);
    v->write("nHead", nHead);
}

} // namespace dspu
} // namespace lsp
