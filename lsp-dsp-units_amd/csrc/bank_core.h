// The host side of a bank of `channels` units that keeps a parameter table and a state array per channel on the device, written
// once (host only, no virtual functions).  Every error text starts with the name of the C entry that reports it, so the entries
// pass their names in.
//
//   check_rows()       what every sample entry asks of its rows: none missing, a count below the entry's limit, strides no
//                      shorter than the rows, in place only with equal strides
//   tables<P, S>       channels, the host copy of the table, its dirty range and the two device arrays; open(), alloc(),
//                      release(), upload(), and the checks of get_params() / get_state() / set_state()
//   settings_bank      tables plus the setters' values and a "needs update" flag per channel: update_settings over the flagged
//                      channels, set_params, create / destroy / clear
//
// A settings bank is  struct mi_<x>_bank : mi_bank::settings_bank<settings, params, device state>  with, as static members:
//     NAME                                 "mi_<x>_bank", as upload_dirty's messages have it
//     fresh_settings(), fresh_params()     a channel as construct() leaves it
//     fresh_state()                        ... and its state on the device
//     compute(settings, params)            update_settings of one channel
// A bank whose update is its own (pending edits of the state, rings that grow, a settings kernel) derives from tables alone.
#pragma once
#include "mi_common.h"

#include <initializer_list>
#include <new>
#include <vector>

namespace mi_bank
{
    enum { REQUIRED = 1, OUTPUT = 2 };
    // a pointer argument of a sample entry: rows of `length` samples, `stride` floats apart
    struct row { const void *p; size_t stride, length; uint32_t flags; };

    // In this order: a REQUIRED row is there; count < limit; unless the bank has one channel, no stride of a row that is there is
    // shorter than the row; an OUTPUT that is also an input has the input's stride.  The rows live on the caller's stack.
    inline int check_rows(const char *entry, uint32_t channels, size_t count, size_t limit, std::initializer_list<row> rows)
    {
        for (const row &r : rows)
            MI_REQUIRE(r.p != nullptr || !(r.flags & REQUIRED), MI_EINVAL, "%s: NULL buffer", entry);
        MI_REQUIRE(count < limit, MI_EINVAL, "%s: count %zu too large", entry, count);
        for (const row &r : rows)
            MI_REQUIRE(channels == 1 || r.p == nullptr || r.stride >= r.length, MI_EINVAL,
                       "%s: stride %zu shorter than the row's %zu samples (count %zu)", entry, r.stride, r.length, count);
        for (const row &o : rows)
            for (const row &i : rows)
                MI_REQUIRE(!(o.flags & OUTPUT) || (i.flags & OUTPUT) || o.p == nullptr || o.p != i.p || o.stride == i.stride, MI_EINVAL,
                           "%s: in place with different strides (%zu, %zu; count %zu)", entry, o.stride, i.stride, count);
        return MI_OK;
    }

    template <class Params, class State> struct tables
    {
        uint32_t                channels = 0;
        std::vector<Params>     params;                 // what the device table holds, or will after the upload
        mi::dirty_range         up;                     // where params differs from the device table
        Params                 *d_params = nullptr;     // [channels]
        State                  *d_state = nullptr;      // [channels]
    };

    // What every create() opens with, in two halves, so that a bank can check its further arguments between them (they are
    // refused with or without a device).  After open_new() *bank is the new, empty bank; whoever fails later destroys it and
    // leaves *bank NULL.
    template <class Bank> int open_checks(Bank **bank, const char *entry, uint32_t channels, uint32_t most = 1u << 20)
    {
        MI_REQUIRE(bank != nullptr, MI_EINVAL, "%s: NULL result pointer", entry);
        *bank = nullptr;
        MI_REQUIRE(channels > 0 && channels <= most, MI_EINVAL, "%s: channels must be 1 .. %u", entry, most);
        return MI_OK;
    }
    template <class Bank> int open_new(Bank **bank, const char *entry)
    {
        MI_REQUIRE(mi_dspu_device_count() > 0, MI_ENODEV, "no HIP device available (there is no CPU fallback)");
        *bank = new (std::nothrow) Bank();
        MI_REQUIRE(*bank != nullptr, MI_ENOMEM, "%s: out of host memory", entry);
        return MI_OK;
    }
    template <class Bank> int open(Bank **bank, const char *entry, uint32_t channels, uint32_t most = 1u << 20)
    {
        const int r = open_checks(bank, entry, channels, most);
        return (r != MI_OK) ? r : open_new(bank, entry);
    }

    template <class Params, class State> void release(tables<Params, State> &b)
    {
        (void)hipFree(b.d_params); (void)hipFree(b.d_state);
        b.d_params = nullptr, b.d_state = nullptr;
    }

    // the table and the state array of b.channels channels, every channel fresh, on the host and on the device
    template <class Params, class State>
    int alloc(tables<Params, State> &b, const char *entry, const Params &fresh_params, const State &fresh_state)
    {
        b.params.assign(b.channels, fresh_params);
        const std::vector<State> states(b.channels, fresh_state);
        const size_t params_bytes = size_t(b.channels) * sizeof(Params), state_bytes = size_t(b.channels) * sizeof(State);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.d_params), params_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&b.d_state), state_bytes);
        if (e == hipSuccess) e = hipMemcpy(b.d_params, b.params.data(), params_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(b.d_state, states.data(), state_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            return MI_OK;
        release(b);
        return mi::fail(MI_EHIP, "%s: %s", entry, hipGetErrorString(e));
    }

    // the changed stretch of the table goes to the device, outside a capture
    template <class Params, class State> int upload(tables<Params, State> &b, const char *name, hipStream_t st)
    {
        return mi::upload_dirty(name, b.d_params, b.params.data(), b.up, st);
    }

    // what a per-channel getter checks before it writes to *out
    template <class Bank> int get_checks(const Bank *b, const char *entry, uint32_t channel, const void *out)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels && out != nullptr, MI_EINVAL, "%s: bad argument", entry);
        return MI_OK;
    }
    template <class Bank, class Params> int get_params(const Bank *b, const char *entry, uint32_t channel, Params *params)
    {
        const int r = get_checks(b, entry, channel, params);
        if (r == MI_OK)
            *params = b->params[channel];
        return r;
    }

    // one channel's device state, from and to the host (`valid`: what the bank asks of the values it is given)
    template <class Bank, class State> int get_state(Bank *b, const char *entry, uint32_t channel, State *s, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_REQUIRE(channel < b->channels, MI_EINVAL, "%s: channel %u out of range", entry, channel);
        return mi::read_state(s, b->d_state + channel, mi::as_stream(stream));
    }
    template <class Bank, class State> int set_state(Bank *b, const char *entry, uint32_t channel, const State &s, bool valid, hipStream_t st)
    {
        MI_REQUIRE(b != nullptr && channel < b->channels && valid, MI_EINVAL, "%s: bad argument", entry);
        return mi::write_state(b->d_state + channel, s, st);
    }

    template <class Settings, class Params, class State> struct settings_bank : tables<Params, State>
    {
        std::vector<Settings>   cfg;                    // the setters' values
        std::vector<uint8_t>    update;                 // bUpdate of every channel
    };

    // update_settings of every channel whose bUpdate is set; the changed stretch of the table goes to the device
    template <class Bank> int update(Bank *b, hipStream_t st)
    {
        for (uint32_t ch = 0; ch < b->channels; ++ch)
        {
            if (!b->update[ch])
                continue;
            Bank::compute(b->cfg[ch], b->params[ch]);
            b->update[ch] = 0;
            b->up.touch(ch);
        }
        return upload(*b, Bank::NAME, st);
    }

    template <class Bank> int update_settings(Bank *b, const char *entry, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        return update(b, mi::as_stream(stream));
    }

    // The computed parameters of one channel, set as they stand.  In two halves, so that a bank can check more of *p between them.
    template <class Bank, class Params> int set_params_checks(Bank *b, const char *entry, uint32_t channel, const Params *p)
    {
        MI_REQUIRE(b != nullptr && p != nullptr && channel < b->channels, MI_EINVAL, "%s: bad argument", entry);
        return MI_OK;
    }
    template <class Bank, class Params> int set_params_store(Bank *b, uint32_t channel, const Params *p)
    {
        if (b->update[channel] == 0 && memcmp(&b->params[channel], p, sizeof(*p)) == 0)
            return MI_OK;
        b->params[channel] = *p;
        b->update[channel] = 0;
        b->up.touch(channel);
        return MI_OK;
    }
    template <class Bank, class Params> int set_params(Bank *b, const char *entry, uint32_t channel, const Params *p)
    {
        const int r = set_params_checks(b, entry, channel, p);
        return (r != MI_OK) ? r : set_params_store(b, channel, p);
    }

    template <class Bank> int destroy(Bank *b)
    {
        if (b == nullptr)
            return MI_OK;
        release(*b);
        delete b;
        return MI_OK;
    }

    template <class Bank> int create(Bank **bank, const char *entry, uint32_t channels)
    {
        int r = open(bank, entry, channels);
        if (r != MI_OK)
            return r;
        Bank *b = *bank;
        b->channels = channels;
        b->cfg.assign(channels, Bank::fresh_settings());
        b->update.assign(channels, 1);
        r = alloc(*b, entry, Bank::fresh_params(), Bank::fresh_state());
        if (r != MI_OK)
        {
            *bank = nullptr;
            destroy(b);
        }
        return r;
    }

    template <class Bank> int clear(Bank *b, const char *entry, void *stream)
    {
        MI_REQUIRE(b != nullptr, MI_ESTATE, "%s: NULL bank", entry);
        MI_HIP_CHECK(hipMemsetAsync(b->d_state, 0, size_t(b->channels) * sizeof(*b->d_state), mi::as_stream(stream)));
        return MI_OK;
    }
} // namespace mi_bank
