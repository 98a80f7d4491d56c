// What the lsp::dspu class wrappers of this directory share on the host side of the device: three pieces, no layer -- the
// callers keep calling mi_*_bank_* themselves.
//
//   rows             the one growable [rows][cap] float buffer on the device that a wrapper stages its blocks in.  Its bounds
//                    are kept here and nowhere else: row(k) is the only place that computes a row's address.
//   registry<Entry>  the one table of state kept BESIDE an object of a class that has no member to hang it on (its bytes are
//                    the reference's): keyed by the object's address, an entry is made at the first call that needs the device
//                    and dropped in destroy() and in construct().  An object whose storage is released without destroy() or
//                    its destructor leaves its entry behind until an object of the class is constructed at that address again.
//   beside<>         the entry of most classes: a bank of one channel, its rows and the bank's state as the device holds it.
//
// rows alone: the impl and handle structs behind pData of Oversampler (two, its base and oversampled lengths differ),
// TruePeakMeter, DynamicDelay and Oscillator, the thread-local staging of Velvet and of the LCG/MLS noise classes, and in
// dspu_classes.cpp `staging`, the gain rows of DynamicFilters and Delay and the impls of MultiSpectralProcessor, LoudnessMeter
// and ILUFSMeter.  registry with an entry of their own: Sidechain and Limiter.  registry<beside<>>: Compressor, Expander, Gate,
// DynamicProcessor, AutoGain, SimpleAutoGain, Correlometer, Panometer, PeakMeter, SurgeProtector, Bypass, Crossfade, Depopper,
// ADSREnvelope, MeterGraph, ScaledMeterGraph and QuantizedCounter.
#pragma once
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>

#include "mi_dspu.h"

namespace mi_host
{
    // Grows, never shrinks, and keeps no contents across a reallocation: every caller stages a block anew after reserve().
    // up() and down() are plain copies on the null stream; neither synchronises, that stays with the caller.
    class rows
    {
        float  *d_buf = nullptr;            // [held][cap]
        size_t  cap = 0, held = 0;

    public:
        rows() {}
        rows(const rows &) = delete;
        rows &operator=(const rows &) = delete;
        ~rows() { release(); }

        size_t capacity() const { return cap; }             // floats in a row: the stride that the banks are told
        size_t nrows() const { return held; }

        // room for k rows of n floats; after a failure the buffer is empty and a later call may succeed
        bool reserve(size_t n, size_t k = 1)
        {
            if (n <= cap && k <= held)
                return true;
            release();
            if (mi_dspu_malloc(reinterpret_cast<void **>(&d_buf), k * n * sizeof(float)) != MI_OK)
            {
                d_buf = nullptr;
                return false;
            }
            cap = n, held = k;
            return true;
        }

        float *row(size_t k) const { return d_buf + k * cap; }

        bool up(size_t k, const float *src, size_t n) const { return mi_dspu_copy_h2d(row(k), src, n * sizeof(float), nullptr) == MI_OK; }
        bool down(float *dst, size_t k, size_t n) const { return mi_dspu_copy_d2h(dst, row(k), n * sizeof(float), nullptr) == MI_OK; }

        void release()
        {
            mi_dspu_free(d_buf);
            d_buf = nullptr;
            cap = held = 0;
        }
    };

    // The table of one class.  An entry's destructor releases what the entry owns (its bank, its rows).
    template <class Entry> class registry
    {
        std::mutex lock;
        std::unordered_map<const void *, Entry *> table;

        static registry &all()
        {
            static registry r;
            return r;
        }

    public:
        typedef Entry entry;

        static Entry *find(const void *self)
        {
            registry &r = all();
            std::lock_guard<std::mutex> guard(r.lock);
            auto it = r.table.find(self);
            return (it != r.table.end()) ? it->second : nullptr;
        }

        // the entry of self, made at the first call: make(entry &) fills a fresh one and returns MI_OK, or nothing is stored
        // and the next call tries again
        template <class Make> static Entry *of(const void *self, Make make)
        {
            registry &r = all();
            std::lock_guard<std::mutex> guard(r.lock);
            auto it = r.table.find(self);
            if (it != r.table.end())
                return it->second;
            Entry *p = new (std::nothrow) Entry();
            if (p == nullptr)
                return nullptr;
            if (make(*p) != MI_OK)
            {
                delete p;
                return nullptr;
            }
            r.table[self] = p;
            return p;
        }

        // ... for the banks whose create takes the channels only: one channel
        template <class Bank> static Entry *of_one(const void *self, int (*create)(Bank **, uint32_t))
        {
            return of(self, [create](Entry &e) { return create(&e.bank, 1); });
        }

        static void drop(const void *self)
        {
            registry &r = all();
            Entry *p = nullptr;
            {
                std::lock_guard<std::mutex> guard(r.lock);
                auto it = r.table.find(self);
                if (it == r.table.end())
                    return;
                p = it->second;
                r.table.erase(it);
            }
            delete p;                                           // outside the lock: it destroys a bank
        }
    };

    // the follower's state of the envelope dynamics (fEnvelope, fPeak, nHoldCounter)
    struct follow_held { float e = 0.0f, peak = 0.0f; uint32_t hold = 0; };

    // Held: the bank's state as the device holds it -- a fresh bank's, then what process() read back -- in 32-bit fields
    // without padding, so that two of them are compared as bytes (a float that was written is sent even where it compares equal)
    template <class Bank, class Held, int (*Destroy)(Bank *)> struct beside
    {
        Bank   *bank = nullptr;
        rows    buf;
        Held    held = Held();

        beside() {}
        beside(const beside &) = delete;
        beside &operator=(const beside &) = delete;
        ~beside()                                               // the bank first, then buf's own destructor
        {
            if (bank != nullptr)
                Destroy(bank);
        }

        // the object's state as the bank's, where its fields are not what the device holds: send(bank, now) sets channel 0's
        template <class Send> bool hand_over_state(const Held &now, Send send)
        {
            if (memcmp(&now, &held, sizeof(Held)) == 0)
                return true;
            if (send(bank, now) != MI_OK)
                return false;
            held = now;
            return true;
        }
    };
} // namespace mi_host
