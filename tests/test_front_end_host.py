"""CPU-side tests of the Python front end's option plumbing (no GPU needed).

 * the public decode methods keep the signatures they had before the pick arguments were bundled;
 * `_fill_options` puts what the caller gave into a GenerateOptions / QueueOptions, read back through the struct's pointers;
 * generate_greedy / generate_sample / generate_penalized leave the legacy entry point exactly when an optional argument is given;
 * the ValueErrors that need no device are raised.
"""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import wrk

# str(inspect.signature(...)) of each method at the commit before the pick bundle
SIGNATURES = {
    "generate_greedy": """(self, first_tokens, steps: 'int', mode: 'int' = 1, want_logits: 'bool' = False, groups: 'int' = 1, logprobs=None, grammar: "'Grammar'" = None, grammar_state=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "'LogitBias'" = None, bias_set=None)""",
    "generate_sample": """(self, first_tokens, steps: 'int', temperature=1.0, top_p=0.5, seed=None, mode: 'int' = 1, want_logits: 'bool' = False, groups: 'int' = 1, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "'LogitBias'" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_penalized": """(self, first_tokens, steps: 'int', occurrence: "'Occurrence'", temperature=1.0, top_p=0.5, seed=None, presence=0.0, frequency=0.0, decay=1.0, mode: 'int' = 1, want_logits: 'bool' = False, groups: 'int' = 1, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "'LogitBias'" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_stop": """(self, first_tokens, steps: 'int', stop, temperature=None, top_p=None, seed=None, occurrence: "'Occurrence'" = None, presence=0.0, frequency=0.0, decay=1.0, mode: 'int' = 1, want_logits: 'bool' = False, groups: 'int' = 1, poll_steps: 'int' = 0, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, stop_sequences=None, stop_tail=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "'LogitBias'" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_guided": """(self, first_tokens, steps: 'int', guidance_scale, negative_first_tokens=None, stop=None, temperature=None, top_p=None, seed=None, occurrence: "'Occurrence'" = None, presence=0.0, frequency=0.0, decay=1.0, mode: 'int' = 1, want_logits: 'bool' = False, poll_steps: 'int' = 0, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, stop_sequences=None, stop_tail=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "'LogitBias'" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_queue": """(self, requests, stop=None, max_new=16, temperature=None, top_p=None, seed=None, occurrence: "'Occurrence'" = None, presence=0.0, frequency=0.0, decay=1.0, init_state: "'Buffer'" = None, max_steps=None, poll_steps: 'int' = 0, mode: 'int' = 1, top_k=None, min_p=None, pool: "'StatePool'" = None, start_state=None, save_state=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, stop_sequences=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, count_prompt=None, history: "'HistoryPool'" = None, logit_bias: "'LogitBias'" = None, bias_set=None, guidance_scale=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_queue_guided": """(self, requests, negative_prompts, guidance_scale, negative_init_state: "'Buffer'" = None, stop=None, max_new=16, temperature=None, top_p=None, seed=None, occurrence: "'Occurrence'" = None, presence=0.0, frequency=0.0, decay=1.0, init_state: "'Buffer'" = None, max_steps=None, poll_steps: 'int' = 0, mode: 'int' = 1, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "'Grammar'" = None, grammar_state=None, stop_sequences=None, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, count_prompt=None, logit_bias: "'LogitBias'" = None, bias_set=None, num_slots=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None)""",
    "generate_beam": """(self, first_tokens, steps: 'int', num_beams: 'int', stop=None, length_penalty: 'float' = 0.0, logit_bias: "'LogitBias'" = None, bias_set=None, mode: 'int' = 1, poll_steps: 'int' = 0, guidance_scale=None, occurrence: "'Occurrence'" = None, presence=0.0, frequency=0.0, decay=1.0, window: "'TokenWindow'" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, grammar: "'Grammar'" = None, grammar_state=None)""",
    "sample_logits": """(self, logits, temperature=1.0, top_p=0.5, seed=0, step: 'int' = 0, num_vocab: 'Optional[int]' = None, top_k=None, min_p=None, mirostat=None, typical_p=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None, row_stride: 'Optional[int]' = None)""",
}

OPTIONS = [wrk.GenerateOptions, wrk.QueueOptions]
CUT_FIELDS = ("top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc_probability", "xtc_threshold")
HANDLE = types.SimpleNamespace(h=0x1000)       # an Occurrence / Grammar / TokenWindow / LogitBias as the builder sees it


def pointer_fields(cls):
    return [name for name, ty in cls._fields_ if ty in (wrk._P, wrk._u32p, wrk._f32p)]


def back(ptr, n):
    """The n values behind a struct's pointer field."""
    assert ptr, "NULL"
    return np.ctypeslib.as_array(ptr, (n,)).copy()


def fill(cls, n, guidance_scale=None, negative_first_tokens=None, **given):
    opt, keep = cls(), []
    ret = wrk._fill_options(opt, wrk._pick(given), n, keep, guidance_scale, negative_first_tokens)
    return opt, ret, keep


def test_public_signatures_are_frozen():
    for name, want in SIGNATURES.items():
        owner = wrk.Context if name == "sample_logits" else wrk.Runtime
        assert str(inspect.signature(getattr(owner, name))) == want, name
    for name in ("generate_stop", "generate_guided", "generate_queue"):
        par = inspect.signature(getattr(wrk.Runtime, name)).parameters
        assert [k for k in wrk._PICK_NAMES if k not in par] == [], name
    assert len(set(wrk._PICK_NAMES)) == len(wrk._PICK_NAMES)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_nothing_given_sets_nothing(cls, n):
    opt, ret, keep = fill(cls, n)
    assert ret == (None, None, None) and keep == []
    assert [f for f in pointer_fields(cls) if getattr(opt, f)] == []
    assert opt.num_dry_breakers == 0


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_scalars_broadcast_and_lists_are_taken_as_given(cls, n):
    top_p, min_p, freq = [0.25, 0.5, 0.75][:n], [0.01, 0.02, 0.03][:n], [0.1, 0.2, 0.3][:n]
    opt, (mu, states, cut_ptrs), _ = fill(cls, n, temperature=0.7, top_p=top_p, seed=9, occurrence=HANDLE, presence=0.5, frequency=freq,
                                          decay=0.9, top_k=5, min_p=min_p, typical_p=0.8, window=HANDLE, dry=(0.8, 1.75, [2, 3, 4][:n]),
                                          no_repeat_ngram=3, dry_breakers=[7, 8], logit_bias=HANDLE, bias_set=[0, wrk.BIAS_NONE, 2][:n],
                                          guidance_scale=1.5)
    assert (mu, states, cut_ptrs) == (None, None, None)
    want = {"temperature": [0.7] * n, "top_p": top_p, "seed": [9] * n, "presence": [0.5] * n, "frequency": freq, "decay": [0.9] * n,
            "top_k": [5] * n, "min_p": min_p, "typical_p": [0.8] * n, "dry_multiplier": [0.8] * n, "dry_base": [1.75] * n,
            "dry_allowed_length": [2, 3, 4][:n], "no_repeat_ngram": [3] * n, "bias_set": [0, wrk.BIAS_NONE, 2][:n], "guidance_scale": [1.5] * n}
    for name, values in want.items():
        got = back(getattr(opt, name), n)
        assert got.dtype == (np.uint32 if dict(cls._fields_)[name] is wrk._u32p else np.float32), name
        np.testing.assert_array_equal(got, np.asarray(values, got.dtype), err_msg=name)
    np.testing.assert_array_equal(back(opt.dry_breakers, 2), [7, 8])
    assert opt.num_dry_breakers == 2
    assert opt.occ == opt.window == opt.bias == HANDLE.h and not opt.grammar
    assert not opt.mirostat_tau and not opt.mirostat_eta and not opt.mirostat_mu and not opt.grammar_state


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_sampler_defaults(cls, n):
    opt, _, _ = fill(cls, n, temperature=0.7)                   # temperature alone: top_p 0.5, seed[i] = i
    np.testing.assert_array_equal(back(opt.temperature, n), np.full(n, 0.7, np.float32))
    np.testing.assert_array_equal(back(opt.top_p, n), np.full(n, 0.5, np.float32))
    np.testing.assert_array_equal(back(opt.seed, n), [0, 1, 2][:n])
    assert not opt.occ and not opt.presence and not opt.top_k and not opt.min_p and not opt.typical_p
    for given in (dict(top_k=4), dict(seed=3), dict(typical_p=0.9), dict(occurrence=HANDLE), dict(eta_cutoff=0.01)):
        opt, _, _ = fill(cls, n, **given)                       # any sampler argument: temperature 1.0
        np.testing.assert_array_equal(back(opt.temperature, n), np.ones(n, np.float32))
        np.testing.assert_array_equal(back(opt.top_p, n), np.full(n, 0.5, np.float32))
        np.testing.assert_array_equal(back(opt.seed, n), [3] * n if "seed" in given else [0, 1, 2][:n])
    opt, _, _ = fill(cls, n, occurrence=HANDLE)                 # the penalties' own defaults
    for name, v in (("presence", 0.0), ("frequency", 0.0), ("decay", 1.0)):
        np.testing.assert_array_equal(back(getattr(opt, name), n), np.full(n, v, np.float32))
    opt, _, _ = fill(cls, n, grammar=HANDLE, window=HANDLE, logit_bias=HANDLE)     # no sampler argument: still the arg-max
    assert not opt.temperature and not opt.top_p and not opt.seed


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_mirostat_mu_is_the_array_the_struct_points_to(cls, n):
    opt, (mu, _, _), _ = fill(cls, n, mirostat=(5, 0.1))
    np.testing.assert_array_equal(mu, np.full(n, 10, np.float32))
    assert mu.dtype == np.float32 and C.addressof(opt.mirostat_mu.contents) == mu.ctypes.data
    np.testing.assert_array_equal(back(opt.mirostat_tau, n), np.full(n, 5, np.float32))
    np.testing.assert_array_equal(back(opt.mirostat_eta, n), np.full(n, 0.1, np.float32))
    np.testing.assert_array_equal(back(opt.temperature, n), np.ones(n, np.float32))
    start = np.asarray([3.0, 4.0, 5.0][:n], np.float32)
    opt, (mu, _, _), _ = fill(cls, n, mirostat=(5, 0.1), mirostat_mu=start)
    np.testing.assert_array_equal(mu, start)
    assert C.addressof(opt.mirostat_mu.contents) == mu.ctypes.data != start.ctypes.data     # a writable copy, not the caller's array


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_cuts_go_into_the_struct_or_come_back(cls, n):
    eps = [0.001, 0.002, 0.003][:n]
    opt, (_, _, cut_ptrs), _ = fill(cls, n, xtc=(0.5, 0.1), epsilon_cutoff=eps)
    ns, ep, eta, prob, thr = cut_ptrs
    assert ns is None and eta is None
    np.testing.assert_array_equal(back(ep, n), np.asarray(eps, np.float32))
    np.testing.assert_array_equal(back(prob, n), np.full(n, 0.5, np.float32))
    np.testing.assert_array_equal(back(thr, n), np.full(n, 0.1, np.float32))
    np.testing.assert_array_equal(back(opt.temperature, n), np.ones(n, np.float32))     # a sampled pick either way
    if cls is wrk.QueueOptions:
        assert [f for f in CUT_FIELDS if hasattr(opt, f)] == []
    else:
        assert not opt.top_n_sigma and not opt.eta_cutoff
        np.testing.assert_array_equal(back(opt.epsilon_cutoff, n), np.asarray(eps, np.float32))
        np.testing.assert_array_equal(back(opt.xtc_probability, n), np.full(n, 0.5, np.float32))
        np.testing.assert_array_equal(back(opt.xtc_threshold, n), np.full(n, 0.1, np.float32))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cls", OPTIONS)
def test_grammar_state_and_bias_set(cls, n):
    for given, want in ((None, [0] * n), (4, [4] * n), ([6, 0, 9][:n], [6, 0, 9][:n])):
        opt, (_, states, _), _ = fill(cls, n, grammar=HANDLE, grammar_state=given)
        np.testing.assert_array_equal(states, want)
        assert states.dtype == np.uint32 and C.addressof(opt.grammar_state.contents) == states.ctypes.data and opt.grammar == HANDLE.h
    opt, _, _ = fill(cls, n, logit_bias=HANDLE)
    assert opt.bias == HANDLE.h and not opt.bias_set                # NULL: the ABI's "set 0 for every row"


def test_negative_first_tokens_go_with_the_guidance():
    opt, _, _ = fill(wrk.GenerateOptions, 3, guidance_scale=[1.0, 2.0, 0.5], negative_first_tokens=[4, 5, 6])
    np.testing.assert_array_equal(back(opt.guidance_scale, 3), np.asarray([1.0, 2.0, 0.5], np.float32))
    np.testing.assert_array_equal(back(opt.guidance_first_tokens, 3), [4, 5, 6])


@pytest.fixture()
def runtime():
    """A Runtime that has no model: every call below must be decided before the device is needed."""
    rt = object.__new__(wrk.Runtime)
    rt.num_batch = 2
    return rt


def test_value_errors_before_any_device_call(runtime):
    for cls in OPTIONS:
        with pytest.raises(ValueError, match="^mirostat_mu without mirostat$"):
            fill(cls, 3, mirostat_mu=1.0)
        with pytest.raises(ValueError, match=r"^xtc = \(probability, threshold\)$"):
            fill(cls, 3, xtc=(0.5,))
    with pytest.raises(ValueError, match="^mirostat_mu without mirostat$"):
        runtime.generate_sample([1, 2], 3, mirostat_mu=1.0)
    with pytest.raises(ValueError, match=r"^xtc = \(probability, threshold\)$"):
        runtime.generate_queue([[1], [2]], xtc=(0.5, 0.1, 0.2))
    for call in (runtime.generate_stop, lambda *a, **kw: runtime.generate_guided(*a[:2], 1.5, stop=a[2], **kw)):
        with pytest.raises(ValueError, match="^stop_tail without stop_sequences$"):
            call([1, 2], 3, [0], stop_tail=[[1], [2]])
    for given in (dict(start_state=0), dict(save_state=[0, 1]), dict(save_state=1, top_n_sigma=1.0)):
        with pytest.raises(ValueError, match="^start_state / save_state need a pool$"):
            runtime.generate_queue([[1], [2]], **given)


LOOP_ARGUMENTS = ("self", "first_tokens", "steps", "mode", "want_logits", "groups")


@pytest.mark.parametrize("name", ["greedy", "sample", "penalized"])
def test_any_optional_argument_leaves_the_legacy_entry_point(runtime, name):
    method = getattr(wrk.Runtime, "generate_" + name)
    runtime._generate = lambda entry, *a: ("legacy", entry)
    runtime._generate_filtered = lambda first_tokens, steps, pick, *a: ("options", pick)
    own = (HANDLE,) if name == "penalized" else ()
    assert method(runtime, [1, 2], 3, *own) == ("legacy", name)
    par = [p for p in inspect.signature(method).parameters if p not in LOOP_ARGUMENTS]
    assert [p for p in par if p not in wrk._PICK_NAMES] == []          # every other argument is a pick argument
    optional = [p for p in par if p not in wrk._PLAIN[name]]
    assert len(optional) == {"greedy": 9, "sample": 18, "penalized": 18}[name]
    for p in optional:
        where, pick = method(runtime, [1, 2], 3, *own, **{p: 1})
        assert where == "options" and pick[p] == 1, p
        assert not wrk._is_plain(pick, wrk._PLAIN[name])
    plain = {"temperature": 0.3, "top_p": 0.9, "seed": [4, 5], "presence": 0.1, "frequency": 0.2, "decay": 0.5}
    plain = {k: v for k, v in plain.items() if k in par}
    assert method(runtime, [1, 2], 3, *own, **plain) == ("legacy", name)      # the entry point's own arguments keep it
