// A bank of one channel and a staging buffer BESIDE an object of a class that has no member to hang them on (its bytes are
// the reference's): they live in a table keyed by the object's address, made at the first call that needs the device and
// dropped in destroy() and in construct().  An object whose storage is released without destroy() or its destructor leaves
// its entry behind until an object of the class is constructed at that address again.  The Compressor, Expander, Gate,
// DynamicProcessor, AutoGain and SimpleAutoGain classes use it.
#pragma once
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>

#include "mi_dspu.h"

namespace mi_host
{
    // the follower's state of the envelope dynamics (fEnvelope, fPeak, nHoldCounter)
    struct follow_held { float e = 0.0f, peak = 0.0f; uint32_t hold = 0; };

    // Held: the bank's state as the device holds it -- a fresh bank's, then what process() read back -- in 32-bit fields
    // without padding, so that two of them are compared as bytes (a float that was written is sent even where it compares equal)
    template <class Bank, class Held> struct beside
    {
        Bank   *bank = nullptr;
        float  *d_buf = nullptr;            // [rows][cap]
        size_t  cap = 0, rows = 0;
        Held    held = Held();

        bool reserve(size_t n, size_t nrows)
        {
            if (n <= cap && nrows <= rows)
                return true;
            mi_dspu_free(d_buf);
            d_buf = nullptr;
            cap = rows = 0;
            if (mi_dspu_malloc(reinterpret_cast<void **>(&d_buf), nrows * n * sizeof(float)) != MI_OK)
                return false;
            cap = n, rows = nrows;
            return true;
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

    // the table of one class, with the bank's create and destroy
    template <class Bank, class Held, int (*Create)(Bank **, uint32_t), int (*Destroy)(Bank *)> class registry
    {
        std::mutex lock;
        std::unordered_map<const void *, beside<Bank, Held> *> table;

        static registry &all()
        {
            static registry r;
            return r;
        }

    public:
        typedef beside<Bank, Held> entry;

        static entry *of(const void *self)
        {
            registry &r = all();
            std::lock_guard<std::mutex> guard(r.lock);
            auto it = r.table.find(self);
            if (it != r.table.end())
                return it->second;
            entry *p = new (std::nothrow) entry();
            if (p == nullptr)
                return nullptr;
            if (Create(&p->bank, 1) != MI_OK)
            {
                delete p;
                return nullptr;
            }
            r.table[self] = p;
            return p;
        }

        static void drop(const void *self)
        {
            registry &r = all();
            entry *p = nullptr;
            {
                std::lock_guard<std::mutex> guard(r.lock);
                auto it = r.table.find(self);
                if (it == r.table.end())
                    return;
                p = it->second;
                r.table.erase(it);
            }
            Destroy(p->bank);
            mi_dspu_free(p->d_buf);
            delete p;
        }
    };
} // namespace mi_host
