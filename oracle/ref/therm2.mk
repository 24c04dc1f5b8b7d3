# oracle/ref/therm2.mk -- builds oracle/_ref/<CFG>/ref_therm2: the reference's own linear_itd (with fit_line), add_new_ice (with
# update_vertical_tracers and the mushy liquidus of ice_therm_mushy), lateral_melt (ice_therm_itd, compiled UNMODIFIED AND WHOLE) and
# aggregate_area, reduce_area, cleanup_itd (ice_itd), with the recipe of oracle/ref/Makefile (its MODS, KMODS, DEFS, FC, FFLAGS:
# -ffp-contract=off), from the sources where they lie, linked with our driver oracle/ref/ref_therm2.F90.  Nothing is copied into this
# repository; every output goes to oracle/_ref/, which is git-ignored.  Test infrastructure: it produces the fixtures
# tests/golden/ref_litd_*.npz and ref_therm2_*.npz (tests/golden/make_ref_therm2.py).
#   make -f therm2.mk CFG=name NX=.. NY=.. BX=.. BY=.. MXB=.. NCAT=..
# Compile order: MODS, KMODS (cpl_parameters, cpl_arrays_setup), ice_zbgc_shared, serial/ice_timers, ice_therm_mushy, the ice_zbgc
# slice, ice_therm_itd.
#
# The ice_zbgc slice: add_new_ice `use`s add_new_ice_bgc of ice_zbgc and nothing else of it, while the module as a whole reaches
# ice_read_write, ice_flux, ice_algae, ice_brine and with them netCDF.  The slice is the module's head (its `use` lines up to
# `contains`) and add_new_ice_bgc through `end module`, cut by line range at build time into oracle/_ref/; after cpp the module's
# `private` and `public :: <list>` lines become one `public` (the list names routines that are not in the slice).  ZBGC_GUARD lists
# "file:line:keyword:name" -- the statement expected on that line, keyword and routine name only -- and the build stops if the
# reference has drifted.  add_new_ice_bgc is never called by the driver's cases (tr_brine and skl_bgc are false in them).
include Makefile

therm2: $(OUT)/ref_therm2
.DEFAULT_GOAL := therm2

ZBGC = source/ice_zbgc.F90
ZBGC_RANGES = $(ZBGC):10:24 $(ZBGC):861:1077
ZBGC_GUARD  = $(ZBGC):10:module:ice_zbgc $(ZBGC):18:private: $(ZBGC):24:contains: $(ZBGC):33:subroutine:init_zbgc \
              $(ZBGC):866:subroutine:add_new_ice_bgc $(ZBGC):1073:end.subroutine:add_new_ice_bgc $(ZBGC):1077:end.module:ice_zbgc
ZBGC_ROUTINES = add_new_ice_bgc
TMODS = source/ice_zbgc_shared serial/ice_timers source/ice_therm_mushy

$(OUT)/ref_therm2: ref_therm2.F90 therm2.mk Makefile
	@test -d $(REF)/source || { echo "oracle/_ref: $(REF) is not present (it never is on the GPU box): nothing to build"; exit 1; }
	@for g in $(ZBGC_GUARD); do f=$${g%%:*}; r=$${g#*:}; n=$${r%%:*}; r=$${r#*:}; kw=$$(echo $${r%%:*} | tr . ' '); nm=$${r#*:}; \
	  sed -n "$${n}p" $(REF)/$$f | grep -qiE "^ *$$kw *$$nm *(\(|&|$$)" || \
	    { echo "oracle/ref: the reference has drifted: $$f line $$n is not '$$kw $$nm'; re-derive ZBGC_RANGES / ZBGC_GUARD"; exit 1; }; done
	@for r in $(ZBGC_RANGES); do f=$${r%%:*}; r=$${r#*:}; a=$${r%%:*}; b=$${r#*:}; \
	  sed -n "$${a}p" $(REF)/$$f | grep -qiE "^ *(module |!=====|$$)" && sed -n "$${b}p" $(REF)/$$f | grep -qiE "^ *(contains|end module)" || \
	    { echo "oracle/ref: the reference has drifted: $$f lines $$a-$$b do not start / end on a statement boundary"; exit 1; }; done
	@mkdir -p $(OUT)/t
	@set -e; cd $(OUT)/t; trap 'cd ..; rm -rf t' EXIT; objs=""; \
	for m in $(MODS) $(KMODS) $(TMODS); do b=$$(basename $$m); \
	  cpp -P -traditional $(DEFS) $(REF)/$$m.F90 > $$b.f90; \
	  $(FC) $(FFLAGS) -w -c $$b.f90 -o $$b.o; objs="$$objs $$b.o"; done; \
	for r in $(ZBGC_RANGES); do f=$${r%%:*}; r=$${r#*:}; sed -n "$${r%%:*},$${r#*:}p" $(REF)/$$f; done > zbgc_slice.F90; \
	got=$$(grep -iE "^ *subroutine " zbgc_slice.F90 | sed -E "s/^ *subroutine +([a-z_0-9]+).*/\1/I" | tr '\n' ' '); \
	test "$$got" = "$(ZBGC_ROUTINES) " || { echo "oracle/ref: the slice holds [$$got], expected [$(ZBGC_ROUTINES)]"; exit 1; }; \
	cpp -P -traditional $(DEFS) zbgc_slice.F90 | \
	  sed -E -e 's/^( *)private *$$/\1public/' -e ':a' -e '/^ *public *::.*& *$$/{N;s/\n/ /;ba;}' -e '/^ *public *::/d' > zbgc_slice.f90; \
	if grep -qiE "^ *(public *::|init_history_bgc *,)" zbgc_slice.f90; then echo "oracle/ref: the public list survived the sed"; exit 1; fi; \
	$(FC) $(FFLAGS) -w -c zbgc_slice.f90 -o zbgc_slice.o; \
	cpp -P -traditional $(DEFS) $(REF)/source/ice_therm_itd.F90 > ice_therm_itd.f90; \
	$(FC) $(FFLAGS) -w -c ice_therm_itd.f90 -o ice_therm_itd.o; \
	$(FC) $(FFLAGS) -w -I. -c $(CURDIR)/ref_therm2.F90 -o ref_therm2.o; \
	$(FC) -o ../ref_therm2 ref_therm2.o ice_therm_itd.o zbgc_slice.o $$objs
	@echo "built $(OUT)/ref_therm2"
