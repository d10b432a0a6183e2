!===============================================================================
! mc_chain -- ONE Markov chain driven exactly like the reference's MonteCarloLoop, with the engine
! behind the reference-named seams of module maniac_gpu (the B = 1 drop-in of INTEGRATION.md).
!
! The control flow, the bookkeeping and -- deliberately -- the ORDER in which random numbers are drawn
! follow the reference statement by statement, so that with the same seed (seed_rng rule,
! src/random_utils.f90:35-56) and the same Fortran runtime the chain visits the same states as the
! reference and writes the same files:
!   MonteCarloLoop                    src/monte_carlo.f90:26-88
!   PickRandomResidueType / PickRandomMoleculeIndex   src/monte_carlo_utils.f90:136-182
!   Translation / RandomTranslation   src/translation.f90:36-112
!   Rotation / ApplyRandomRotation / ChooseRotationAngle   src/rotation.f90:34-75,
!                                     src/monte_carlo_utils.f90:30-92
!   CreateMolecule / InsertAndOrientMolecule / Accept / Reject   src/create_molecule.f90:41-207
!   DeleteMolecule / RemoveMolecule / Accept / Reject            src/delete_molecule.f90:41-199
!   ComputeOldEnergy / ComputeNewEnergy / AcceptMove             src/monte_carlo_utils.f90:275-422
!   mc_acceptance_probability         src/monte_carlo_utils.f90:184-226
!   AdjustMoveStepSizes               src/monte_carlo_utils.f90:99-130 (as written)
!   ApplyPBC                          src/geometry_utils.f90:167-213
! Differences from the reference, both deliberate (SURVEY F2 / F3): A(k) is initialised to S(k) by
! ComputeSystemEnergy, and a deletion's new reciprocal energy removes the deleted molecule.
! mchain_set_as_written(1) selects the reference's deletion exactly as written instead (F3): DeleteMolecule
! compacts first (RemoveMolecule: slot m <- last slot, delete_molecule.f90:99-116) and ComputeNewEnergy then calls
! ComputeRecipEnergySingleMol with is_creation = deletion_flag (monte_carlo_utils.f90:308), so A(k) GAINS the
! terms of the molecule now sitting in slot m and keeps them when the move is accepted.  That mode lives in
! this host loop only: it is composed from the engine's neutral primitives (a creation-kind reciprocal energy
! of the swapped-in molecule's sites; on acceptance mgpu_replica_replace_molecule, mgpu_replica_set_num_molecules
! and mgpu_structure_factor_add) -- no kernel knows about it.  Intended physics stays the default.
! Energies are evaluated against the engine's resident state; nothing is saved or restored on
! rejection (the reference's Save/RestoreSingleMolFourier have no counterpart).
!
! Every mode takes a step through the same three stages, each written once:
!   DRAW      draw_step: the reference's order of random numbers and the conditions under which a draw is skipped, into a
!             step_draws record of raw uniforms.  The chain runs push such records as they are; build_trial forms the trial
!             geometry from one for the paths that build on the host.
!   EVALUATE  one routine per way of asking the engine, each giving the rows o / w (w2) and a verdict: evaluate_seams,
!             evaluate_batch (a window of steps, or one), evaluate_launch (the one-launch window), and the collect of a
!             chain run (run_block).
!   RESOLVE   energy_states (old / new from the rows), acceptance_prefactor + accepts (the rule), count_trial,
!             book_accepted, reservoir_take / reservoir_give, commit_as_written, commit_step; resolve_step strings them
!             together for a step built on the host, run_block books a collected record with the same pieces.
! The mode variables (fused, spec_k, chain_cap, run_on, run_gc) choose the evaluator in mchain_run and take_steps only.
!===============================================================================
module mc_chain

    use, intrinsic :: iso_c_binding
    use, intrinsic :: iso_fortran_env, only: real64
    use maniac_gpu
    use maniac_output
    use mc_farm, only: mfarm_set_output_template

    implicit none

    private
    public :: mchain_reset, mchain_set_box, mchain_set_residue, mchain_set_bonded, mchain_set_tables, &
              mchain_set_moves, mchain_set_reservoir_box, mchain_set_reservoir_residue, mchain_run, &
              mchain_get_energy, mchain_get_counters, mchain_get_counts, mchain_get_molecule, mchain_get_steps, &
              mchain_set_mode, mchain_set_as_written, mchain_set_log_header, mchain_write_log_header, &
              mchain_set_speculation, mchain_set_chain_windows, mchain_set_wide_windows, mchain_get_loop_seconds, mchain_get_times, &
              mchain_export_template, mchain_set_chain_run, mchain_get_chain_run, mchain_set_chain_run_gcmc, &
              mchain_get_chain_run_gcmc

    real(real64), parameter :: PI = 3.14159265358979323846_real64, TWOPI = 2.0_real64 * PI
    real(real64), parameter :: zero = 0.0_real64, one = 1.0_real64, half = 0.5_real64, three = 3.0_real64
    ! src/parameters.f90:8, :14-21
    integer, parameter :: NB_MAX_MOLECULE = 5000
    real(real64), parameter :: TARGET_ACCEPTANCE = 0.40d0, TOL_ACCEPTANCE = 0.05d0
    real(real64), parameter :: MIN_TRANSLATION_STEP = 1.0d-3, MAX_TRANSLATION_STEP = 3.0d0
    real(real64), parameter :: MIN_ROTATION_ANGLE = 1.0d-3, MAX_ROTATION_ANGLE = 0.78d0
    real(real64), parameter :: PROB_CREATE_DELETE = 0.5d0
    integer, parameter :: MIN_TRIALS_FOR_RECALIBRATION = 500
    integer, parameter :: TYPE_CREATION = 1, TYPE_DELETION = 2, TYPE_TRANSLATION = 3, TYPE_ROTATION = 4

    type(chain_block), save, target :: S
    integer, save :: status = 0          ! first engine error met (0 = none); the loop stops on it
    ! .true.: one batched engine call per move (mgpu_gcmc_trial_submit / wait with one candidate, resident-row
    ! commit) instead of one call per reference seam -- same energies, a third of the launches and waits
    logical, save :: fused = .true.
    ! .true.: the reference's deletion update as written (SURVEY F3); see the header
    logical, save :: as_written = .false.
    ! the messages the reference logs before the Monte Carlo loop (banner, input echo, data-file summary,
    ! Lorentz-Berthelot listing, Ewald parameters), one per line, prepared by the front end (io_maniac.log_header_lines)
    character(len=:), allocatable, save :: log_header
    ! Speculative window (fused mode): the next spec_k steps are drawn in the reference's random-number order ASSUMING
    ! every one of them is rejected -- the state then does not change, so all their trials are trials from the current
    ! state and are evaluated in ONE batched engine call.  The window is then walked in order with the saved acceptance
    ! draws; the first accepted step is applied, the generator is put back to its state right after that step's draws
    ! and the rest of the window is thrown away.  Visited states, random stream and files are those of the sequential
    ! loop; the engine round trips per step drop by up to 1 / acceptance.  spec_k = 1: the sequential loop.
    integer, save :: spec_k = 1
    integer, parameter :: STEP_NOOP = -1, STEP_ABORT = -2
    ! One launch per window (mgpu_chain_window): the engine evaluates the window's steps, applies the acceptance rule to
    ! them in order with the draws saved here and commits the first accepted step itself; a step whose draw is too close
    ! to its probability for two exp implementations to be sure to agree comes back UNDECIDED and is decided (and
    ! committed) by this loop.  chain_windows: wanted (default); chain_cap: the engine's window capacity, 0 = the engine
    ! cannot (triclinic box, large molecules) and the window goes through mgpu_gcmc_trial_submit / wait as before.
    logical, save :: chain_windows = .true.
    ! wide_windows: one-launch windows also for rigid molecules of 6 to 63 sites (mgpu_chain_set_wide); off unless asked for
    logical, save :: wide_windows = .false.
    integer, save :: chain_cap = 0
    ! Chain runs (mchain_set_chain_run; include/maniac_gpu.h mgpu_chain_run_*): an NVT block's steps are drawn ahead as records of
    ! draws -- nothing is built here and nothing is ever rewound -- and the engine runs them in launches queued back to back,
    ! each continuing from the cursor it finds; this loop keeps run_depth launches in flight and books the results in order.
    ! run_k = 0: off (the default).  run_on: the mode applies to this run (set by mchain_run from the engine's capacity).
    integer, save :: run_k = 0, run_depth = 3
    logical, save :: run_on = .false.
    ! Grand-canonical chain runs (mchain_set_chain_run_gcmc; mgpu_chain_run_set_gc, mgpu_chain_run_push_gc): a block with exchange
    ! moves runs as a chain run of by-count records (run_block, by_count).  run_gc_want: the host asked; run_gc: it applies to this run;
    ! run_fallback: steps of the last mchain_run taken through the windows because the ahead-of-outcome rule failed.
    ! Orthorhombic boxes, and triclinic ones whose engine has triclinic runs on (mgpu_chain_run_set_triclinic); never with a
    ! reservoir or as_written.
    logical, save :: run_gc_want = .false., run_gc = .false.
    integer, save :: run_fallback = 0
    integer(c_int), save :: run_ring = 0
    integer, parameter :: BY_HOST = -1, DEVICE_REJECTED = 0, DEVICE_ACCEPTED = 1
    ! time spent inside the Monte Carlo loop proper (no initial energy, no files), seconds
    real(real64), save :: loop_seconds = 0.0_real64
    ! ... in ComputeSystemEnergy before the loop, and in the output files (UpdateFiles, PrintStatus)
    real(real64), save :: init_seconds = 0.0_real64, file_seconds = 0.0_real64

    ! how an accepted step that the host decided reaches the engine (commit_step): set by the evaluator that was used
    integer, parameter :: COMMIT_SEAM = 1, COMMIT_ROWS = 2, COMMIT_SITES = 3

    ! One step as drawn (draw_step): its type, kind (MGPU_* or STEP_*) and move type, and the raw uniforms.  A chain run
    ! pushes these as they are; build_trial forms a proposal's geometry from them.
    type :: step_draws
        integer :: t = 0, m = 0, kind = STEP_NOOP, mtype = 0   ! m: the slot `sel` picks from the count at the draw (creation: count + 1)
        real(real64) :: sel = 0.0_real64                ! the molecule draw itself
        real(real64) :: pos(3) = 0.0_real64             ! displacement, or an insertion's position
        real(real64) :: angle = 0.0_real64, axis = 0.0_real64
        real(real64) :: pick = 0.0_real64               ! the reservoir molecule an insertion copies
        real(real64) :: u = 0.0_real64                  ! acceptance
    end type step_draws
    type :: proposal
        type(step_draws) :: d
        integer :: cand = 0, cand2 = 0                  ! rows of the batch (cand2: the second row of an as-written deletion)
        integer :: pick = 0                             ! reservoir molecule an insertion copies
        real(real64) :: com(3) = 0.0_real64
        real(real64), allocatable :: off(:, :)          ! (3, n1)
        integer, allocatable :: rng(:)                  ! generator state after the step's draws (windows only)
    end type proposal
    ! the window's candidate list as handed to the engine (kept for the resident-row commit)
    integer(c_int), allocatable, save :: w_rep(:), w_t(:), w_m(:), w_kind(:), w_acc(:), w_link(:)
    real(c_double), allocatable, save :: w_u(:), w_pref(:)
    integer, save :: w_stride = 1

contains

    ! rand_uniform / rand_symmetric (src/random_utils.f90:13-31)
    function rand_uniform() result(v)
        real(real64) :: v
        call random_number(v)
    end function rand_uniform

    subroutine seed_rng(seed)
        integer, intent(in) :: seed
        integer :: n, i
        integer, allocatable :: put(:)
        call random_seed(size=n)
        allocate(put(n))
        put = seed + 37 * [(i - 1, i = 1, n)]
        call random_seed(put=put)
    end subroutine seed_rng

    subroutine note(stat)
        integer, intent(in) :: stat
        if (stat /= 0 .and. status == 0) status = stat
    end subroutine note

    !---------------------------------------------------------------------------
    ! Building the state (called from the host plumbing, in this order: reset, box, residues,
    ! bonded tables, tables, moves, reservoir)
    !---------------------------------------------------------------------------
    subroutine mchain_reset(engine, n_res, n_atom_types, temperature) bind(C, name="mchain_reset")
        type(c_ptr), value :: engine
        integer(c_int), value :: n_res, n_atom_types
        real(c_double), value :: temperature
        call blank_chain(S)
        S%engine = engine
        S%n_res = n_res
        S%n_atom_types = n_atom_types
        S%temperature = temperature
        allocate(S%res(n_res), S%rsv(n_res), S%masses(n_atom_types))
        S%masses = zero
        status = 0
    end subroutine mchain_reset

    subroutine blank_chain(c)
        type(chain_block), intent(out) :: c            ! intent(out): every component back to its default
        c%engine = c_null_ptr
    end subroutine blank_chain

    subroutine fill_box(b, matrix, reciprocal, lo, hi, tilt, is_triclinic, box_type, volume)
        type(box_block), intent(out) :: b
        real(c_double), intent(in) :: matrix(3, 3), reciprocal(3, 3), lo(3), hi(3), tilt(3), volume
        integer(c_int), intent(in) :: is_triclinic, box_type
        b%matrix = matrix
        b%reciprocal = reciprocal
        b%lo = lo
        b%hi = hi
        b%tilt = tilt
        b%is_triclinic = is_triclinic /= 0
        b%box_type = box_type
        b%volume = volume
        b%num_atoms = 0
    end subroutine fill_box

    ! matrix / reciprocal are the Fortran arrays box%matrix / box%reciprocal (column-major)
    subroutine mchain_set_box(matrix, reciprocal, lo, hi, tilt, is_triclinic, box_type, volume) &
            bind(C, name="mchain_set_box")
        real(c_double), intent(in) :: matrix(3, 3), reciprocal(3, 3), lo(3), hi(3), tilt(3)
        integer(c_int), value :: is_triclinic, box_type
        real(c_double), value :: volume
        call fill_box(S%box, matrix, reciprocal, lo, hi, tilt, is_triclinic, box_type, volume)
    end subroutine mchain_set_box

    subroutine mchain_set_reservoir_box(matrix, reciprocal, lo, hi, tilt, is_triclinic, box_type, volume, &
                                        any_bonded) bind(C, name="mchain_set_reservoir_box")
        real(c_double), intent(in) :: matrix(3, 3), reciprocal(3, 3), lo(3), hi(3), tilt(3)
        integer(c_int), value :: is_triclinic, box_type
        real(c_double), value :: volume
        integer(c_int), intent(in) :: any_bonded(4)
        call fill_box(S%rbox, matrix, reciprocal, lo, hi, tilt, is_triclinic, box_type, volume)
        S%has_reservoir = .true.
        S%any_bonded = any_bonded /= 0
    end subroutine mchain_set_reservoir_box

    subroutine fill_residue(r, n1, cap, count, com, off)
        type(residue_block), intent(inout) :: r
        integer, intent(in) :: n1, cap, count
        real(c_double), intent(in) :: com(3, *), off(3, n1, *)
        integer :: m
        r%n1 = n1
        r%cap = max(cap, count, 1)
        r%count = count
        if (allocated(r%com)) deallocate(r%com, r%off)
        allocate(r%com(3, r%cap), r%off(3, n1, r%cap))
        r%com = zero
        r%off = zero
        do m = 1, count
            r%com(:, m) = com(:, m)
            r%off(:, :, m) = off(:, :, m)
        end do
    end subroutine fill_residue

    subroutine mchain_set_residue(t, name, n1, active, cap, count, atom_type, charge, com, off, fugacity) &
            bind(C, name="mchain_set_residue")
        integer(c_int), value :: t, n1, active, cap, count
        character(kind=c_char), intent(in) :: name(*)
        integer(c_int), intent(in) :: atom_type(n1)
        real(c_double), intent(in) :: charge(n1), com(3, *), off(3, n1, *)
        real(c_double), value :: fugacity
        integer :: i
        associate (r => S%res(t))
            r%name = ''
            do i = 1, 10
                if (name(i) == c_null_char) exit
                r%name(i:i) = name(i)
            end do
            r%active = active
            r%atom_type = atom_type
            r%charge = charge
            r%fugacity = fugacity
            call fill_residue(r, int(n1), int(cap), int(count), com, off)
            S%box%num_atoms = S%box%num_atoms + count * n1
        end associate
    end subroutine mchain_set_residue

    subroutine mchain_set_reservoir_residue(t, n1, cap, count, com, off) bind(C, name="mchain_set_reservoir_residue")
        integer(c_int), value :: t, n1, cap, count
        real(c_double), intent(in) :: com(3, *), off(3, n1, *)
        call fill_residue(S%rsv(t), int(n1), int(cap), int(count), com, off)
        S%rbox%num_atoms = S%rbox%num_atoms + count * n1
    end subroutine mchain_set_reservoir_residue

    ! kind 1 bonds, 2 angles, 3 dihedrals, 4 impropers; table(1, k) = type, table(2:, k) = local atom indices
    subroutine mchain_set_bonded(t, kind, n, table) bind(C, name="mchain_set_bonded")
        integer(c_int), value :: t, kind, n
        integer(c_int), intent(in) :: table(5, *)
        integer, allocatable :: grown(:, :, :)
        integer :: k
        associate (r => S%res(t))
            if (.not. allocated(r%bonded)) then
                allocate(r%bonded(5, max(1, n), 4))
                r%bonded = 0
            else if (size(r%bonded, 2) < n) then
                allocate(grown(5, n, 4))
                grown = 0
                grown(:, 1:size(r%bonded, 2), :) = r%bonded
                call move_alloc(grown, r%bonded)
            end if
            r%n_bonded(kind) = n
            do k = 1, n
                r%bonded(:, k, kind) = table(:, k)
            end do
        end associate
    end subroutine mchain_set_bonded

    subroutine mchain_set_tables(masses, n_bonded_types) bind(C, name="mchain_set_tables")
        real(c_double), intent(in) :: masses(*)
        integer(c_int), intent(in) :: n_bonded_types(4)
        S%masses = masses(1:S%n_atom_types)
        S%n_bonded_types = n_bonded_types
    end subroutine mchain_set_tables

    subroutine mchain_set_moves(translation_step, rotation_step, p_translation, p_rotation, recalibrate) &
            bind(C, name="mchain_set_moves")
        real(c_double), value :: translation_step, rotation_step, p_translation, p_rotation
        integer(c_int), value :: recalibrate
        S%translation_step = translation_step
        S%rotation_step = rotation_step
        S%p_translation = p_translation
        S%p_rotation = p_rotation
        S%recalibrate = recalibrate /= 0
    end subroutine mchain_set_moves

    !---------------------------------------------------------------------------
    ! Geometry helpers
    !---------------------------------------------------------------------------
    subroutine apply_pbc(pos, box)
        real(real64), intent(inout) :: pos(3)
        type(box_block), intent(in) :: box
        real(real64) :: frac(3)
        integer :: d
        if (.not. box%is_triclinic) then
            do d = 1, 3
                pos(d) = box%lo(d) + modulo(pos(d) - box%lo(d), box%matrix(d, d))
            end do
        else
            frac = matmul(box%reciprocal, pos - box%lo)
            do d = 1, 3
                frac(d) = modulo(frac(d), one)
            end do
            pos = box%lo + matmul(box%matrix, frac)
        end if
    end subroutine apply_pbc

    ! RotationMatrix (src/helper_utils.f90:39-77)
    function axis_rotation(axis, theta) result(r)
        integer, intent(in) :: axis
        real(real64), intent(in) :: theta
        real(real64) :: r(3, 3), c, sn
        integer :: p, q
        c = cos(theta)
        sn = sin(theta)
        r = zero
        r(1, 1) = one; r(2, 2) = one; r(3, 3) = one
        ! the plane (p, q) the axis leaves invariant: x -> (2,3), y -> (3,1), z -> (1,2)
        p = mod(axis, 3) + 1
        q = mod(axis + 1, 3) + 1
        if (axis >= 1 .and. axis <= 3) then
            r(p, p) = c; r(p, q) = -sn
            r(q, p) = sn; r(q, q) = c
        end if
    end function axis_rotation

    !---------------------------------------------------------------------------
    ! Evaluators.  Each hands back the engine's rows of a step, e = non_coulomb, coulomb, recip, self, intra: o of the
    ! molecule where it is, w of the trial (w2: the second row of an as-written deletion).
    ! The seams: the reference-named calls one by one, in the order ComputeOldEnergy and ComputeNewEnergy make them; the
    ! old state is the mirror's slot m, the new one the proposal's geometry.
    !---------------------------------------------------------------------------
    subroutine evaluate_seams(p, o, w, w2)
        type(proposal), intent(in) :: p
        real(real64), intent(out) :: o(5), w(5), w2(5)
        integer :: t, m, n1, last, stat
        t = p%d%t
        m = p%d%m
        n1 = S%res(t)%n1
        o = zero
        w = zero
        w2 = zero
        select case (p%d%kind)
        case (MGPU_MOVE)
            call ComputeRecipEnergySingleMol(S%engine, t, m, S%res(t)%com(:, m), S%res(t)%off(:, 1:n1, m), n1, o(IE_RECIP), stat=stat)
            call note(stat)
            call ComputePairInteractionEnergy_singlemol(S%engine, t, m, S%res(t)%com(:, m), S%res(t)%off(:, 1:n1, m), n1, &
                                                        o(IE_NONC), o(IE_COUL), stat=stat)
            call note(stat)
            call ComputeRecipEnergySingleMol(S%engine, t, m, p%com, p%off, n1, w(IE_RECIP), stat=stat)
            call note(stat)
            call ComputePairInteractionEnergy_singlemol(S%engine, t, m, p%com, p%off, n1, w(IE_NONC), w(IE_COUL), stat=stat)
            call note(stat)
        case (MGPU_CREATION)
            call ComputeRecipEnergySingleMol(S%engine, t, m, p%com, p%off, n1, w(IE_RECIP), is_creation=.true., stat=stat)
            call note(stat)
            ! (exclude nothing: the engine does not hold the molecule yet)
            call ComputePairInteractionEnergy_singlemol(S%engine, t, 0, p%com, p%off, n1, w(IE_NONC), w(IE_COUL), stat=stat)
            call note(stat)
            call ComputeEwaldSelfInteractionSingleMol(S%engine, t, w(IE_SELF), stat=stat)
            call note(stat)
            call ComputeIntraResidueRealCoulombEnergySingleMol(S%engine, t, m, p%com, p%off, n1, w(IE_INTRA), stat=stat)
            call note(stat)
        case (MGPU_DELETION)
            call ComputePairInteractionEnergy_singlemol(S%engine, t, m, p%com, p%off, n1, o(IE_NONC), o(IE_COUL), stat=stat)
            call note(stat)
            call ComputeEwaldSelfInteractionSingleMol(S%engine, t, o(IE_SELF), stat=stat)
            call note(stat)
            call ComputeIntraResidueRealCoulombEnergySingleMol(S%engine, t, m, p%com, p%off, n1, o(IE_INTRA), stat=stat)
            call note(stat)
            ! the system without the molecule (the engine still holds it in slot m)
            call ComputeRecipEnergySingleMol(S%engine, t, m, p%com, p%off, n1, w(IE_RECIP), is_deletion=.true., stat=stat)
            call note(stat)
            if (as_written) then
                ! ComputeNewEnergy as written (monte_carlo_utils.f90:301-309): after RemoveMolecule slot m holds the
                ! former last molecule, and the reciprocal update runs with is_creation = .true. on that slot
                last = S%res(t)%count
                call ComputeRecipEnergySingleMol(S%engine, t, last, S%res(t)%com(:, last), S%res(t)%off(:, 1:n1, last), n1, &
                                                 w2(IE_RECIP), is_creation=.true., stat=stat)
                call note(stat)
            end if
        end select
    end subroutine evaluate_seams

    ! seams /= 0: call the reference-named seams one by one (the literal integration of INTEGRATION.md section 3)
    subroutine mchain_set_mode(seams) bind(C, name="mchain_set_mode")
        integer(c_int), value :: seams
        fused = seams == 0
    end subroutine mchain_set_mode

    ! text = the header messages separated by line feeds (n bytes; n = 0 clears it)
    subroutine mchain_set_log_header(text, n) bind(C, name="mchain_set_log_header")
        integer(c_int), value :: n
        character(kind=c_char), intent(in) :: text(*)
        integer :: i
        if (allocated(log_header)) deallocate(log_header)
        if (n <= 0) return
        allocate(character(len=n) :: log_header)
        do i = 1, n
            log_header(i:i) = text(i)
        end do
    end subroutine mchain_set_log_header

    ! every header message through the reference's list-directed write (LogMessage, output_utils.f90:30-36)
    subroutine write_log_header(ch)
        type(chain_block), intent(in) :: ch
        if (allocated(log_header)) call log_text(ch, log_header)
    end subroutine write_log_header

    ! The chain's static description (box, residue templates and inactive residues, bonded lists, masses, reservoir box) as
    ! the output template of the selected farm (mfarm_write_block): a farm of replicas of this input writes its files with
    ! this chain's writers
    subroutine mchain_export_template() bind(C, name="mchain_export_template")
        call mfarm_set_output_template(S)
    end subroutine mchain_export_template

    ! Test hook (no engine needed): write the header alone to `path`
    subroutine mchain_write_log_header(path) bind(C, name="mchain_write_log_header")
        character(kind=c_char), intent(in) :: path(*)
        character(len=512) :: p
        integer :: i
        type(chain_block) :: tmp
        p = ''
        do i = 1, len(p)
            if (path(i) == c_null_char) exit
            p(i:i) = path(i)
        end do
        tmp%log_unit = 37
        open(unit=tmp%log_unit, file=trim(p), status='replace')
        call write_log_header(tmp)
        close(tmp%log_unit)
    end subroutine mchain_write_log_header

    ! k > 1: speculative windows of k steps in the batched (non-seams) mode; k <= 1: one step at a time
    subroutine mchain_set_speculation(k) bind(C, name="mchain_set_speculation")
        integer(c_int), value :: k
        spec_k = max(1, min(int(k), 64))
    end subroutine mchain_set_speculation

    ! on /= 0 (default): windows go to the engine's one-launch path where it applies
    subroutine mchain_set_chain_windows(on) bind(C, name="mchain_set_chain_windows")
        integer(c_int), value :: on
        chain_windows = on /= 0
    end subroutine mchain_set_chain_windows

    subroutine mchain_set_wide_windows(on) bind(C, name="mchain_set_wide_windows")
        integer(c_int), value :: on
        wide_windows = on /= 0
    end subroutine mchain_set_wide_windows

    ! k > 0: NVT blocks as chain runs of k steps per launch with `depth` launches in flight, where the engine takes them
    ! (mgpu_chain_run_capacity) and the input has no insertions / deletions; elsewhere the loop keeps its windows.  0: off.
    subroutine mchain_set_chain_run(k, depth) bind(C, name="mchain_set_chain_run")
        integer(c_int), value :: k, depth
        run_k = max(0, int(k))
        run_depth = max(1, int(depth))
    end subroutine mchain_set_chain_run

    ! Chain runs for blocks WITH insertions / deletions (off by default): with this and mchain_set_chain_run on, such a block runs as
    ! a chain run of by-count records where the engine takes it (orthorhombic box, no reservoir) and the run is not --as-written
    ! (whose `link` deletion has no device-built form); elsewhere, and without it, mchain_run decides as it always did.
    subroutine mchain_set_chain_run_gcmc(on) bind(C, name="mchain_set_chain_run_gcmc")
        integer(c_int), value :: on
        run_gc_want = on /= 0
    end subroutine mchain_set_chain_run_gcmc

    ! (gcmc, fallback_steps) of the last mchain_run
    subroutine mchain_get_chain_run_gcmc(out) bind(C, name="mchain_get_chain_run_gcmc")
        integer(c_int), intent(out) :: out(2)
        out = [merge(1_c_int, 0_c_int, run_gc), int(run_fallback, c_int)]
    end subroutine mchain_get_chain_run_gcmc

    ! (on, k, depth) of the last mchain_run
    subroutine mchain_get_chain_run(out) bind(C, name="mchain_get_chain_run")
        integer(c_int), intent(out) :: out(3)
        out = [merge(1_c_int, 0_c_int, run_on), int(run_k, c_int), int(run_depth, c_int)]
    end subroutine mchain_get_chain_run

    function mchain_get_loop_seconds() bind(C, name="mchain_get_loop_seconds") result(sec)
        real(c_double) :: sec
        sec = loop_seconds
    end function mchain_get_loop_seconds

    ! seconds of the last mchain_run: initial energy, Monte Carlo steps, output files
    subroutine mchain_get_times(t) bind(C, name="mchain_get_times")
        real(c_double), intent(out) :: t(3)
        t = [init_seconds, loop_seconds, file_seconds]
    end subroutine mchain_get_times

    subroutine mchain_set_as_written(on) bind(C, name="mchain_set_as_written")
        integer(c_int), value :: on
        as_written = on /= 0
    end subroutine mchain_set_as_written

    !---------------------------------------------------------------------------
    ! DRAW.  One step's random numbers in the order MonteCarloLoop's body and the move drivers draw them: type, molecule,
    ! move, insertion or deletion; then the displacement | the angle, then the axis (ApplyRandomRotation) | the position
    ! with its reservoir pick or its angle and axis; the acceptance draw last.  A step with nothing to do draws nothing
    ! further and stays STEP_NOOP: Translation, Rotation and DeleteMolecule return at once for an empty type, Rotation
    ! for a one-site type.  A creation into a full type is STEP_ABORT (CheckMoleculeIndex aborts the reference there).
    ! The placement of an accepted deletion in the reservoir is drawn after the outcome, by reservoir_give.
    !---------------------------------------------------------------------------
    subroutine draw_step(d)
        type(step_draws), intent(out) :: d
        real(real64) :: draw
        integer :: n, n1
        d%t = pick_residue_type()
        n = S%res(d%t)%count
        n1 = S%res(d%t)%n1
        if (n /= 0) then                                                 ! PickRandomMoleculeIndex
            d%sel = rand_uniform()
            d%m = min(int(d%sel * n) + 1, n)
        end if
        draw = rand_uniform()
        if (draw <= S%p_translation) then
            if (d%m /= 0) then
                d%mtype = TYPE_TRANSLATION
                d%kind = MGPU_MOVE
                call random_number(d%pos)
            end if
        else if (draw <= S%p_rotation + S%p_translation) then
            if (n1 /= 1 .and. d%m /= 0) then
                d%mtype = TYPE_ROTATION
                d%kind = MGPU_MOVE
                d%angle = rand_uniform()
                d%axis = rand_uniform()
            end if
        else if (rand_uniform() <= PROB_CREATE_DELETE) then
            d%m = n + 1
            d%mtype = TYPE_CREATION
            d%kind = STEP_ABORT
            if (d%m <= NB_MAX_MOLECULE .and. d%m <= S%res(d%t)%cap) then
                d%kind = MGPU_CREATION
                call random_number(d%pos)
                if (S%has_reservoir) then
                    call random_number(d%pick)
                else if (n1 /= 1) then
                    d%angle = rand_uniform()
                    d%axis = rand_uniform()
                end if
            end if
        else if (n /= 0) then
            d%mtype = TYPE_DELETION
            d%kind = MGPU_DELETION
        end if
        if (d%kind >= 0) d%u = rand_uniform()
    end subroutine draw_step

    ! The trial geometry of a drawn step, for the paths that build on the host (Translation / RandomTranslation,
    ! ApplyRandomRotation, InsertAndOrientMolecule); the chain's state is not touched.  A deletion's "trial" is the
    ! molecule where it is.
    subroutine build_trial(p)
        type(proposal), intent(inout) :: p
        integer :: t, m, n1, axis
        real(real64) :: trial(3), theta, rot(3, 3)
        logical :: turn
        t = p%d%t
        m = p%d%m
        n1 = S%res(t)%n1
        trial = p%d%pos
        turn = .false.
        if (p%d%mtype == TYPE_CREATION) then
            p%com = S%box%lo + matmul(S%box%matrix, trial)
            if (S%has_reservoir) then
                p%pick = int(p%d%pick * S%rsv(t)%count) + 1
                p%off = S%rsv(t)%off(:, 1:n1, p%pick)
            else
                p%off = S%res(t)%off(:, 1:n1, 1)
                theta = p%d%angle * TWOPI
                turn = n1 /= 1
            end if
        else
            p%com = S%res(t)%com(:, m)
            p%off = S%res(t)%off(:, 1:n1, m)
            if (p%d%mtype == TYPE_TRANSLATION) then
                trial = (trial - half) * S%translation_step
                p%com = S%res(t)%com(:, m) + trial
                call apply_pbc(p%com, S%box)
            else if (p%d%mtype == TYPE_ROTATION) then
                theta = (p%d%angle - half) * S%rotation_step
                turn = .true.
            end if
        end if
        if (turn) then
            axis = int(p%d%axis * three) + 1
            rot = axis_rotation(axis, theta)
            p%off = matmul(rot, p%off)
        end if
    end subroutine build_trial

    !---------------------------------------------------------------------------
    ! EVALUATE (evaluate_seams above; the batched call and the one-launch window here; a chain run's collect in run_block).
    ! add_rows appends a proposal's row(s) to the candidate list w_* and their sites; `stride` = sites per row.
    !---------------------------------------------------------------------------
    subroutine add_rows(p, n_cand, sites, stride)
        type(proposal), intent(inout) :: p
        integer, intent(inout) :: n_cand
        integer, intent(in) :: stride
        real(real64), intent(inout) :: sites(3, stride, *)
        integer :: t, n1, last
        if (.not. allocated(w_rep)) then
            allocate(w_rep(128), w_t(128), w_m(128), w_kind(128), w_acc(128), w_link(128), w_u(128), w_pref(128))
        end if
        t = p%d%t
        n1 = S%res(t)%n1
        w_stride = stride
        n_cand = n_cand + 1
        p%cand = n_cand
        w_rep(n_cand) = 0
        w_t(n_cand) = t - 1
        w_m(n_cand) = p%d%m - 1
        if (p%d%kind == MGPU_CREATION) w_m(n_cand) = -1
        w_kind(n_cand) = p%d%kind
        w_link(n_cand) = -1
        w_u(n_cand) = p%d%u
        w_pref(n_cand) = acceptance_prefactor(t, p%d%mtype)
        call MoleculeSites(p%com, p%off, n1, sites(:, 1:n1, n_cand))
        if (p%d%kind == MGPU_DELETION .and. as_written) then
            ! F3: the reciprocal update runs with is_creation on the molecule RemoveMolecule moves into slot m
            last = S%res(t)%count
            n_cand = n_cand + 1
            p%cand2 = n_cand
            w_link(n_cand - 1) = n_cand - 1                                 ! 0-based row of the companion
            w_rep(n_cand) = 0
            w_t(n_cand) = t - 1
            w_m(n_cand) = -1
            w_kind(n_cand) = MGPU_CREATION
            w_link(n_cand) = -2                                             ! energy only
            w_u(n_cand) = zero
            w_pref(n_cand) = zero
            call MoleculeSites(S%res(t)%com(:, last), S%res(t)%off(:, 1:n1, last), n1, sites(:, 1:n1, n_cand))
        end if
    end subroutine add_rows

    ! the batched call: every row's energies, the rule left to the host (the rows stay resident for COMMIT_ROWS)
    subroutine evaluate_batch(n_cand, sites, o, w)
        integer, intent(in) :: n_cand
        real(real64), intent(in) :: sites(3, w_stride, *)
        real(real64), intent(out) :: o(5, *), w(5, *)
        integer(c_int) :: rc
        rc = mgpu_gcmc_trial_submit(S%engine, 0_c_int, int(n_cand, c_int), w_rep, w_t, w_m, w_kind, sites, int(w_stride, c_int))
        if (rc == MGPU_OK) rc = mgpu_gcmc_trial_wait(S%engine, 0_c_int, o, w)
        call note(int(rc))
    end subroutine evaluate_batch

    ! one launch per window: the engine also applies the rule to the rows in order and commits the first accepted one
    ! (`first`); a row too close to call (`und`) is left to the host.  Both 0-based, -1 = none.
    subroutine evaluate_launch(n_cand, sites, o, w, first, und)
        integer, intent(in) :: n_cand
        real(real64), intent(in) :: sites(3, w_stride, *)
        real(real64), intent(out) :: o(5, *), w(5, *)
        integer(c_int), intent(out) :: first, und
        integer(c_int) :: rc
        rc = mgpu_chain_window(S%engine, 0_c_int, int(n_cand, c_int), w_t, w_m, w_kind, w_link, sites, int(w_stride, c_int), &
                               w_u, w_pref, S%temperature, S%energy(IE_RECIP), o, w, first, und)
        call note(int(rc))
    end subroutine evaluate_launch

    !---------------------------------------------------------------------------
    ! RESOLVE.  The part of Translation / Rotation / CreateMolecule / DeleteMolecule that follows the energy evaluation,
    ! in pieces every path shares.
    !---------------------------------------------------------------------------
    ! ComputeOldEnergy / ComputeNewEnergy: old and new of a move type from the engine's rows
    subroutine energy_states(mtype, o, w, w2, old, new)
        integer, intent(in) :: mtype
        real(real64), intent(in) :: o(5), w(5), w2(5)
        real(real64), intent(out) :: old(6), new(6)
        old = zero
        new = zero
        select case (mtype)
        case (TYPE_CREATION)
            old(IE_RECIP) = S%energy(IE_RECIP)
            new(1:5) = w
        case (TYPE_DELETION)
            old(1:5) = o
            old(IE_RECIP) = S%energy(IE_RECIP)
            new(IE_RECIP) = w(IE_RECIP)
            if (as_written) new(IE_RECIP) = w2(IE_RECIP)                  ! creation-kind energy of the swapped-in molecule (F3)
        case default
            old(1:3) = o(1:3)
            new(1:3) = w(1:3)
        end select
        if (mtype == TYPE_CREATION .or. mtype == TYPE_DELETION) then
            old(IE_TOTAL) = old(IE_NONC) + old(IE_COUL) + old(IE_RECIP) + old(IE_SELF) + old(IE_INTRA)
            new(IE_TOTAL) = new(IE_NONC) + new(IE_COUL) + new(IE_RECIP) + new(IE_SELF) + new(IE_INTRA)
        else
            old(IE_TOTAL) = old(IE_NONC) + old(IE_COUL) + old(IE_RECIP)
            new(IE_TOTAL) = new(IE_NONC) + new(IE_COUL) + new(IE_RECIP)
        end if
    end subroutine energy_states

    ! The factor in front of exp(-delta_e / T) in mc_acceptance_probability (monte_carlo_utils.f90:184-226); n = the type's
    ! count as the move drivers have it when they call the rule: after the insertion, after the removal
    function acceptance_prefactor(t, mtype) result(f)
        integer, intent(in) :: t, mtype
        real(real64) :: f, n, v, phi
        v = S%box%volume
        phi = S%res(t)%fugacity
        select case (mtype)
        case (TYPE_CREATION)
            n = real(S%res(t)%count + 1)
            f = (phi * v / n)
        case (TYPE_DELETION)
            n = real(S%res(t)%count - 1)
            f = ((n + one) / (phi * v))
        case default
            f = one
        end select
    end function acceptance_prefactor

    ! mc_acceptance_probability against the step's acceptance draw u
    function accepts(t, mtype, old, new, u) result(yes)
        integer, intent(in) :: t, mtype
        real(real64), intent(in) :: old(6), new(6), u
        logical :: yes
        real(real64) :: delta_e
        delta_e = new(IE_TOTAL) - old(IE_TOTAL)
        yes = u <= min(one, acceptance_prefactor(t, mtype) * exp(-delta_e / S%temperature))
    end function accepts

    subroutine count_trial(mtype)
        integer, intent(in) :: mtype
        integer, parameter :: TRIAL_OF(4) = [C_TRIAL_C, C_TRIAL_D, C_TRIAL_T, C_TRIAL_R]
        S%counter(TRIAL_OF(mtype)) = S%counter(TRIAL_OF(mtype)) + 1
    end subroutine count_trial

    ! AcceptMove and the Accept of CreateMolecule / DeleteMolecule: running energies, accepted counter, count, num_atoms.
    ! A move touches only the three components it has: adding the zeros of the other two would turn the -0.0 an uncharged
    ! system's self energy can be into +0.0, and energy.dat prints the sign.
    subroutine book_accepted(t, mtype, old, new)
        integer, intent(in) :: t, mtype
        real(real64), intent(in) :: old(6), new(6)
        integer, parameter :: ACCEPTED_OF(4) = [C_C, C_D, C_T, C_R]
        integer :: dn
        if (mtype == TYPE_CREATION .or. mtype == TYPE_DELETION) then
            dn = merge(1, -1, mtype == TYPE_CREATION)
            S%energy(IE_RECIP) = new(IE_RECIP)
            S%energy(IE_SELF) = S%energy(IE_SELF) + new(IE_SELF) - old(IE_SELF)
            S%energy(IE_INTRA) = S%energy(IE_INTRA) + new(IE_INTRA) - old(IE_INTRA)
            S%res(t)%count = S%res(t)%count + dn
            S%box%num_atoms = S%box%num_atoms + dn * S%res(t)%n1
        else
            S%energy(IE_RECIP) = S%energy(IE_RECIP) + new(IE_RECIP) - old(IE_RECIP)
        end if
        S%energy(IE_NONC) = S%energy(IE_NONC) + new(IE_NONC) - old(IE_NONC)
        S%energy(IE_COUL) = S%energy(IE_COUL) + new(IE_COUL) - old(IE_COUL)
        S%energy(IE_TOTAL) = S%energy(IE_TOTAL) + new(IE_TOTAL) - old(IE_TOTAL)
        S%counter(ACCEPTED_OF(mtype)) = S%counter(ACCEPTED_OF(mtype)) + 1
    end subroutine book_accepted

    ! the inserted molecule leaves the reservoir: its slot takes the reservoir's last molecule
    subroutine reservoir_take(t, pick)
        integer, intent(in) :: t, pick
        integer :: n1, last
        n1 = S%res(t)%n1
        last = S%rsv(t)%count
        S%rsv(t)%com(:, pick) = S%rsv(t)%com(:, last)
        S%rsv(t)%off(:, 1:n1, pick) = S%rsv(t)%off(:, 1:n1, last)
        S%rsv(t)%count = S%rsv(t)%count - 1
        S%rbox%num_atoms = S%rbox%num_atoms - n1
    end subroutine reservoir_take

    ! the reservoir receives the geometry the primary box's last slot held, at a place drawn now (after the outcome)
    subroutine reservoir_give(t, off_last)
        integer, intent(in) :: t
        real(real64), intent(in) :: off_last(:, :)
        real(real64) :: trial(3)
        integer :: n1
        n1 = S%res(t)%n1
        call random_number(trial)
        trial = trial - half
        associate (r => S%rsv(t))
            if (r%count + 1 <= r%cap) then
                r%com(:, r%count + 1) = trial(1) * S%rbox%matrix(:, 1) + trial(2) * S%rbox%matrix(:, 2) + &
                                        trial(3) * S%rbox%matrix(:, 3)
                r%off(:, 1:n1, r%count + 1) = off_last(:, 1:n1)
                r%count = r%count + 1
                S%rbox%num_atoms = S%rbox%num_atoms + n1
            else
                call note(4)
            end if
        end associate
    end subroutine reservoir_give

    ! An accepted deletion as written (F3), after the mirror's slot m has taken the former last molecule: coordinates and
    ! count as RemoveMolecule leaves them; A(k) gains the swapped-in molecule's terms and keeps them
    subroutine commit_as_written(t, m, last)
        integer, intent(in) :: t, m, last
        real(real64), allocatable :: sites_last(:, :)
        integer :: n1, stat
        n1 = S%res(t)%n1
        allocate(sites_last(3, n1))
        call MoleculeSites(S%res(t)%com(:, m), S%res(t)%off(:, 1:n1, m), n1, sites_last)
        stat = mgpu_replica_replace_molecule(S%engine, 0_c_int, int(t - 1, c_int), int(m - 1, c_int), int(last - 1, c_int))
        call note(stat)
        stat = mgpu_replica_set_num_molecules(S%engine, 0_c_int, int(t - 1, c_int), int(last - 1, c_int))
        call note(stat)
        stat = mgpu_structure_factor_add(S%engine, 0_c_int, int(t - 1, c_int), sites_last)
        call note(stat)
    end subroutine commit_as_written

    ! An accepted step the host decided reaches the engine the way its evaluator left open: the seam (GpuAcceptMove), the
    ! batch's rows still resident on the lane, or -- after a one-launch window, whose rows are not the lane's -- its sites
    subroutine commit_step(p, how, n_cand)
        type(proposal), intent(in) :: p
        integer, intent(in) :: how, n_cand
        integer(c_int) :: rc, rep(1), tt(1), mm(1), kk(1), acc(1)
        real(real64), allocatable, target :: sites(:, :)
        integer :: n1, stat
        n1 = S%res(p%d%t)%n1
        select case (how)
        case (COMMIT_SEAM)
            call GpuAcceptMove(S%engine, p%d%t, p%d%m, p%d%kind, p%com, p%off, n1, stat=stat)
            call note(stat)
        case (COMMIT_SITES)
            allocate(sites(3, n1))
            call MoleculeSites(p%com, p%off, n1, sites)
            rep = 0; tt = p%d%t - 1; mm = p%d%m - 1; kk = int(p%d%kind, c_int); acc = 1
            if (p%d%kind == MGPU_CREATION) mm = -1
            rc = mgpu_commit_submit(S%engine, 0_c_int, 1_c_int, rep, tt, mm, kk, c_loc(sites), int(n1, c_int), acc)
            call note(int(rc))
        case (COMMIT_ROWS)
            w_acc(1:n_cand) = 0
            w_acc(p%cand) = 1
            rc = mgpu_commit_submit(S%engine, 0_c_int, int(n_cand, c_int), w_rep, w_t, w_m, w_kind, c_null_ptr, &
                                    int(w_stride, c_int), w_acc)
            call note(int(rc))
        end select
    end subroutine commit_step

    ! One evaluated step of a path that builds on the host.  verdict: BY_HOST -- the rule is applied here and an accepted
    ! step is committed through the engine (`how`); DEVICE_REJECTED / DEVICE_ACCEPTED -- the engine has applied the rule
    ! and the commit already.  `restore`: a window may have drawn past this step, so the generator goes back to the state
    ! saved after this step's draws before anything else is drawn.
    subroutine resolve_step(p, o, w, w2, verdict, how, n_cand, restore, accepted)
        type(proposal), intent(in) :: p
        real(real64), intent(in) :: o(5), w(5), w2(5)
        integer, intent(in) :: verdict, how, n_cand
        logical, intent(in) :: restore
        logical, intent(out) :: accepted
        real(real64) :: old(6), new(6)
        real(real64), allocatable :: off_last(:, :)
        integer :: t, m, n1, last, mtype
        t = p%d%t
        m = p%d%m
        mtype = p%d%mtype
        n1 = S%res(t)%n1
        call count_trial(mtype)
        call energy_states(mtype, o, w, w2, old, new)
        if (verdict == BY_HOST) then
            accepted = accepts(t, mtype, old, new, p%d%u)
        else
            accepted = verdict == DEVICE_ACCEPTED
        end if
        if (.not. accepted) return
        if (restore) call random_seed(put=p%rng)
        last = S%res(t)%count
        if (mtype == TYPE_DELETION) then
            off_last = S%res(t)%off(:, :, last)
            S%res(t)%com(:, m) = S%res(t)%com(:, last)                    ! RemoveMolecule: slot m <- the last slot
            S%res(t)%off(:, :, m) = S%res(t)%off(:, :, last)
        else
            S%res(t)%com(:, m) = p%com
            S%res(t)%off(:, 1:n1, m) = p%off
        end if
        call book_accepted(t, mtype, old, new)
        if (verdict == BY_HOST) then
            if (mtype == TYPE_DELETION .and. as_written) then
                call commit_as_written(t, m, last)
            else
                call commit_step(p, how, n_cand)
            end if
        end if
        if (S%has_reservoir .and. mtype == TYPE_CREATION) call reservoir_take(t, p%pick)
        if (S%has_reservoir .and. mtype == TYPE_DELETION) call reservoir_give(t, off_last)
    end subroutine resolve_step

    ! One step of MonteCarloLoop's body: draw, evaluate that step alone -- through the seams, or as a batch of one -- resolve
    subroutine plain_step(batched)
        logical, intent(in) :: batched
        type(proposal) :: p
        real(real64) :: o(5, 2), w(5, 2)
        real(real64), allocatable :: sites(:, :, :)
        integer :: n1, n_cand
        logical :: accepted
        call draw_step(p%d)
        if (p%d%kind == STEP_ABORT) call note(4)
        if (p%d%kind < 0) return
        call build_trial(p)
        n1 = S%res(p%d%t)%n1
        if (p%d%kind == MGPU_CREATION) then
            ! InsertAndOrientMolecule builds the trial in slot count + 1 and a rejection leaves it there: the next insertion
            ! into a type that is still empty copies slot 1 as this one left it
            S%res(p%d%t)%com(:, p%d%m) = p%com
            S%res(p%d%t)%off(:, 1:n1, p%d%m) = p%off
        end if
        o = zero
        w = zero
        if (batched) then
            allocate(sites(3, n1, 2))
            n_cand = 0
            call add_rows(p, n_cand, sites, n1)
            call evaluate_batch(n_cand, sites, o, w)
            call resolve_step(p, o(:, 1), w(:, 1), w(:, 2), BY_HOST, COMMIT_ROWS, n_cand, .false., accepted)
        else
            call evaluate_seams(p, o(:, 1), w(:, 1), w(:, 2))
            call resolve_step(p, o(:, 1), w(:, 1), w(:, 2), BY_HOST, COMMIT_SEAM, 0, .false., accepted)
        end if
    end subroutine plain_step

    !---------------------------------------------------------------------------
    ! Speculative window: up to kwin steps are drawn and built ASSUMING every one of them is rejected, evaluated in one
    ! engine call -- the batched call, or the engine's one-launch window of launch_cap > 0 rows, which also decides -- and walked in order;
    ! returns the number of steps consumed.  The generator's state after a step's draws is kept only here, where the walk
    ! may have to go back to it.
    !---------------------------------------------------------------------------
    function run_window(kwin, launch_cap) result(done)
        integer, intent(in) :: kwin, launch_cap
        integer :: done
        type(proposal), allocatable :: P(:)
        real(real64), allocatable :: sites(:, :, :), o(:, :), w(:, :)
        real(real64) :: none5(5)
        integer :: j, n_prop, n_cand, t, c, mx, verdict, how, nseed
        integer(c_int) :: first, und
        logical :: accepted, one_launch
        one_launch = launch_cap > 0
        mx = 1
        do t = 1, S%n_res
            mx = max(mx, S%res(t)%n1)
        end do
        allocate(P(kwin))
        allocate(sites(3, mx, 2 * kwin), o(5, 2 * kwin), w(5, 2 * kwin))
        sites = zero
        call random_seed(size=nseed)
        n_prop = 0
        n_cand = 0
        do j = 1, kwin
            ! a step may need two rows (as-written deletion): never draw a step the engine's window cannot hold
            if (one_launch .and. n_cand + 2 > launch_cap) exit
            call draw_step(P(j)%d)
            if (kwin > 1) then
                allocate(P(j)%rng(nseed))
                call random_seed(get=P(j)%rng)
            end if
            n_prop = j
            if (P(j)%d%kind == STEP_ABORT) exit
            if (P(j)%d%kind == STEP_NOOP) cycle
            call build_trial(P(j))
            call add_rows(P(j), n_cand, sites, mx)
        end do
        first = -1
        und = -1
        how = COMMIT_ROWS
        if (one_launch) how = COMMIT_SITES
        if (n_cand > 0) then
            if (one_launch) then
                call evaluate_launch(n_cand, sites, o, w, first, und)
            else
                call evaluate_batch(n_cand, sites, o, w)
            end if
        end if
        none5 = zero
        done = n_prop
        do j = 1, n_prop
            if (status /= 0) then
                done = j - 1
                exit
            end if
            if (P(j)%d%kind == STEP_ABORT) then
                call note(4)
                done = j
                exit
            end if
            if (P(j)%d%kind == STEP_NOOP) cycle
            c = P(j)%cand
            verdict = BY_HOST
            if (one_launch) then
                verdict = DEVICE_REJECTED
                if (c - 1 == first) verdict = DEVICE_ACCEPTED
                if (c - 1 == und) verdict = BY_HOST                         ! too close to call on the device: decided here
            end if
            if (P(j)%cand2 > 0) then
                call resolve_step(P(j), o(:, c), w(:, c), w(:, P(j)%cand2), verdict, how, n_cand, j < n_prop, accepted)
            else
                call resolve_step(P(j), o(:, c), w(:, c), none5, verdict, how, n_cand, j < n_prop, accepted)
            end if
            if (accepted) then
                done = j
                exit
            end if
            if (one_launch .and. c - 1 == und) then
                ! rejected here: the engine decided nothing behind this step, so the window ends with it
                if (j < n_prop) call random_seed(put=P(j)%rng)
                done = j
                exit
            end if
        end do
        done = max(done, 1)
    end function run_window

    !---------------------------------------------------------------------------
    ! One block of nb_step steps as a chain run: the steps are drawn ahead and pushed as records of their draws -- the
    ! engine builds the geometry (its construction is the one held to the reference; this file's matmul contracts where the
    ! reference's doubles do not), applies the rule and commits, in launches queued back to back -- so the mirror S%res is
    ! NOT kept in step here: refresh_frames reloads it when the run closes.  This loop keeps run_depth launches in flight
    ! and collects the verdicts in order; a step the engine left undecided is decided here and forced.
    ! by_count: a grand-canonical block.  Its records carry the molecule draw itself (the launch that takes the record
    ! picks the slot from the count it finds), an NVT block's the slot.  How many numbers a step draws depends on the
    ! molecule count at its edges (draw_step), so such a record is drawn AHEAD OF THE OUTCOMES before it only while no
    ! count can reach an edge (ahead_ok).  Where the rule fails with records outstanding they are collected first; where
    ! it fails with none, the run is closed, the mirror refreshed, steps go through the path the loop takes without runs
    ! until it holds again (at least one; counted in run_fallback), the frames are uploaded and the run reopened.
    ! An NVT block's counts never change: its rule always holds, and an empty active type pushes no-op records.
    ! A verdict other than accepted / rejected for a by-count record that was not drawn as a no-op means the engine's count
    ! is not this loop's: an engine-state error.
    !---------------------------------------------------------------------------
    subroutine run_block(nb_step, by_count)
        integer, intent(in) :: nb_step
        logical, intent(in) :: by_count
        integer, parameter :: RUN_MOVE(4) = [3, 4, 1, 2]                    ! the record's move code of a TYPE_*
        integer(c_int), allocatable :: rt(:), rm(:), rmove(:), verdict(:)
        real(c_double), allocatable :: ru(:, :), rau(:), rsel(:), rphi(:), o(:, :), w(:, :)
        integer, allocatable :: mtype(:), n_ins(:), n_del(:)
        type(step_draws) :: d
        real(real64) :: old(6), new(6), none5(5)
        integer :: j, t, pushed, collected, queued, n, i, chunk, done, n0
        integer(c_int) :: rc, n_got, stalled_at
        integer(c_long_long) :: seen0, seen, st_steps, st_void, st_und
        logical :: is_open
        allocate(rt(nb_step), rm(nb_step), rmove(nb_step), mtype(nb_step), ru(5, nb_step), rau(nb_step), rsel(nb_step), rphi(nb_step))
        allocate(n_ins(S%n_res), n_del(S%n_res))
        chunk = 256
        allocate(o(5, chunk), w(5, chunk), verdict(chunk))
        n_ins = 0; n_del = 0
        none5 = zero
        pushed = 0; collected = 0; queued = 0; seen0 = 0
        is_open = .false.
        do while (collected < nb_step .and. status == 0)
            if (pushed == collected .and. .not. ahead_ok()) then
                ! nothing outstanding and a count at an edge
                if (is_open) then
                    rc = mgpu_chain_run_close(S%engine)
                    call note(int(rc))
                    is_open = .false.
                    call refresh_frames()
                end if
                call drop_frames()
                do while (collected < nb_step .and. status == 0)
                    done = take_steps(nb_step - collected)
                    collected = collected + done
                    run_fallback = run_fallback + done
                    if (ahead_ok()) exit
                end do
                pushed = collected
                if (status == 0) call upload_frames()                       ! (the next run, of this block or the next, builds from them)
                cycle
            end if
            if (.not. is_open) then
                rc = mgpu_chain_run_get_stats(S%engine, seen0, st_steps, st_void, st_und)
                call note(int(rc))
                rc = mgpu_chain_run_open(S%engine, 0_c_int, int(run_k, c_int), S%translation_step, S%rotation_step, S%temperature)
                call note(int(rc))
                if (status /= 0) exit
                is_open = .true.
                queued = 0
            end if
            ! records as far ahead as the rule and the ring take them, then launches up to the depth, then the next results in order
            n0 = pushed
            do while (pushed < nb_step .and. pushed - collected < int(run_ring))
                if (.not. ahead_ok()) exit
                call draw_step(d)
                pushed = pushed + 1
                call keep_record(pushed)
            end do
            if (pushed > n0) then
                if (by_count) then
                    rc = mgpu_chain_run_push_gc(S%engine, int(pushed - n0, c_int), rt(n0 + 1:), rmove(n0 + 1:), ru(:, n0 + 1:), &
                                                rau(n0 + 1:), rsel(n0 + 1:), rphi(n0 + 1:))
                else
                    rc = mgpu_chain_run_push(S%engine, int(pushed - n0, c_int), rt(n0 + 1:), rm(n0 + 1:), rmove(n0 + 1:), &
                                             ru(:, n0 + 1:), rau(n0 + 1:))
                end if
                call note(int(rc))
            end if
            rc = mgpu_chain_run_get_stats(S%engine, seen, st_steps, st_void, st_und)
            call note(int(rc))
            n = run_depth - (queued - int(seen - seen0))
            if (n > 0) then
                rc = mgpu_chain_run_launch(S%engine, int(n, c_int))
                call note(int(rc))
                queued = queued + n
            end if
            if (status /= 0) exit
            ! (the engine hands over no more than it was pushed; the two kinds of run have always asked for these two limits)
            n = merge(pushed, nb_step, by_count) - collected
            rc = mgpu_chain_run_collect(S%engine, int(min(chunk, n), c_int), 1_c_int, o, w, verdict, n_got, stalled_at)
            call note(int(rc))
            if (status /= 0) exit
            do i = 1, int(n_got)
                j = collected + 1
                t = int(rt(j)) + 1
                if (verdict(i) == 2) then
                    ! too close to call on the device: this loop's own exp decides, and the engine obeys
                    call energy_states(mtype(j), o(:, i), w(:, i), none5, old, new)
                    rc = mgpu_chain_run_force(S%engine, stalled_at, merge(1_c_int, 0_c_int, accepts(t, mtype(j), old, new, rau(j))))
                    call note(int(rc))
                    queued = queued + 1
                    exit                                                     ! (collected again, with its final verdict)
                end if
                if (mtype(j) /= 0) then
                    if (by_count .and. verdict(i) /= DEVICE_ACCEPTED .and. verdict(i) /= DEVICE_REJECTED) then
                        call note(4)
                        exit
                    end if
                    call count_trial(mtype(j))
                    if (verdict(i) == DEVICE_ACCEPTED) then
                        call energy_states(mtype(j), o(:, i), w(:, i), none5, old, new)
                        call book_accepted(t, mtype(j), old, new)
                    end if
                    if (mtype(j) == TYPE_CREATION) n_ins(t) = n_ins(t) - 1
                    if (mtype(j) == TYPE_DELETION) n_del(t) = n_del(t) - 1
                end if
                collected = j
            end do
        end do
        if (is_open) then
            rc = mgpu_chain_run_close(S%engine)
            call note(int(rc))
            call refresh_frames()                                            ! (the engine's counts must be this loop's: note(4) otherwise)
        end if
    contains
        ! may one more record be drawn before the outstanding ones are decided?  With count_t from the verdicts collected so
        ! far and I_t / D_t the insertion / deletion records pushed and not yet collected: count_t - D_t >= 1 and
        ! count_t + I_t <= min(cap_t, NB_MAX_MOLECULE) - 1 for EVERY active type
        function ahead_ok() result(ok)
            logical :: ok
            integer :: tt
            ok = .true.
            if (.not. by_count) return
            do tt = 1, S%n_res
                if (S%res(tt)%active /= 1) cycle
                if (S%res(tt)%count - n_del(tt) < 1) ok = .false.
                ! a type of more than one site keeps its LAST molecule for the host's path: an insertion copies the geometry the
                ! mirror holds in slot 1 (build_trial), which for an emptied type is the deleted molecule's as it was last moved --
                ! the host's mirror has it, refresh_frames cannot ask the engine for the frame of an empty type
                if (S%res(tt)%n1 /= 1 .and. S%res(tt)%count - n_del(tt) < 2) ok = .false.
                if (S%res(tt)%count + n_ins(tt) > min(S%res(tt)%cap, NB_MAX_MOLECULE) - 1) ok = .false.
            end do
        end function ahead_ok

        ! record jj = the step just drawn, as it is
        subroutine keep_record(jj)
            integer, intent(in) :: jj
            rt(jj) = d%t - 1
            rm(jj) = max(d%m - 1, 0)
            rsel(jj) = d%sel
            ru(1, jj) = d%pos(1)                                         ! (element by element: the compiler hands the
            ru(2, jj) = d%pos(2)                                         ! section's assignment to the runtime, per record)
            ru(3, jj) = d%pos(3)
            ru(4, jj) = d%angle
            ru(5, jj) = d%axis
            rau(jj) = d%u
            rphi(jj) = one
            rmove(jj) = 0
            mtype(jj) = 0
            if (d%kind < 0) return
            mtype(jj) = d%mtype
            rmove(jj) = RUN_MOVE(d%mtype)
            if (d%mtype == TYPE_CREATION .or. d%mtype == TYPE_DELETION) rphi(jj) = S%res(d%t)%fugacity * S%box%volume
            if (d%mtype == TYPE_CREATION) n_ins(d%t) = n_ins(d%t) + 1
            if (d%mtype == TYPE_DELETION) n_del(d%t) = n_del(d%t) + 1
        end subroutine keep_record
    end subroutine run_block

    ! Steps of a block on the host: the evaluator the mode variables choose -- a window of up to `left` steps, or one plain
    ! step; returns the number of steps taken
    function take_steps(left) result(done)
        integer, intent(in) :: left
        integer :: done
        if (fused .and. (spec_k > 1 .or. chain_cap > 0)) then
            ! a window never crosses the end of a block (AdjustMoveStepSizes and the files come there)
            done = run_window(min(spec_k, left), chain_cap)
        else
            call plain_step(fused)
            done = 1
        end if
    end function take_steps


    ! the mirror's frames of the active types from the engine, which built and committed the block's moves
    subroutine refresh_frames()
        integer :: t, n1
        integer(c_int) :: rc, nm
        real(c_double), allocatable :: com(:, :), off(:, :, :)
        do t = 1, S%n_res
            if (S%res(t)%active /= 1 .or. S%res(t)%count == 0) cycle
            n1 = S%res(t)%n1
            allocate(com(3, S%res(t)%count), off(3, n1, S%res(t)%count))
            rc = mgpu_replica_get_frames(S%engine, 0_c_int, int(t - 1, c_int), nm, com, off)
            call note(int(rc))
            if (rc == MGPU_OK .and. int(nm) == S%res(t)%count) then
                S%res(t)%com(:, 1:S%res(t)%count) = com
                S%res(t)%off(:, 1:n1, 1:S%res(t)%count) = off
            else if (rc == MGPU_OK) then
                call note(4)
            end if
            deallocate(com, off)
        end do
    end subroutine refresh_frames

    ! the engine's sites from the mirror, WITHOUT frames: the window path hands over rows built here, which an engine that holds
    ! frames refuses (they would no longer mirror its sites); upload_frames gives them back
    subroutine drop_frames()
        integer :: t, n1, m, n
        integer(c_int) :: rc
        real(c_double), allocatable :: sites(:, :, :)
        do t = 1, S%n_res
            if (S%res(t)%active /= 1) cycle
            n1 = S%res(t)%n1
            n = S%res(t)%count
            allocate(sites(3, n1, max(n, 1)))
            sites = zero
            do m = 1, n
                call MoleculeSites(S%res(t)%com(:, m), S%res(t)%off(:, 1:n1, m), n1, sites(:, :, m))
            end do
            rc = mgpu_replica_set_molecules(S%engine, 0_c_int, int(t - 1, c_int), int(n, c_int), sites)
            call note(int(rc))
            deallocate(sites)
        end do
    end subroutine drop_frames

    ! the engine's frames from the mirror (a chain run builds its moves from them)
    subroutine upload_frames()
        integer :: t, n1
        integer(c_int) :: rc
        do t = 1, S%n_res
            if (S%res(t)%active /= 1) cycle
            n1 = S%res(t)%n1
            rc = mgpu_replica_set_frames(S%engine, 0_c_int, int(t - 1, c_int), int(S%res(t)%count, c_int), &
                                         S%res(t)%com(:, 1:max(S%res(t)%count, 1)), S%res(t)%off(:, 1:n1, 1:max(S%res(t)%count, 1)))
            call note(int(rc))
        end do
    end subroutine upload_frames

    ! AdjustMoveStepSizes, as written -- including the second branches that compare against +TOL and the
    ! rotation step that is multiplied by 1.95 and clamped from above by MIN_ROTATION_ANGLE
    subroutine adjust_move_step_sizes()
        real(real64) :: acc
        if (.not. S%recalibrate) return
        if (S%counter(C_TRIAL_T) > MIN_TRIALS_FOR_RECALIBRATION) then
            acc = real(S%counter(C_T)) / real(S%counter(C_TRIAL_T))
            if (acc - TARGET_ACCEPTANCE > TOL_ACCEPTANCE) then
                S%translation_step = min(S%translation_step * 1.05d0, MAX_TRANSLATION_STEP)
            else if (acc - TARGET_ACCEPTANCE < TOL_ACCEPTANCE) then
                S%translation_step = max(S%translation_step * 0.95d0, MIN_TRANSLATION_STEP)
            end if
        end if
        if (S%counter(C_TRIAL_R) > MIN_TRIALS_FOR_RECALIBRATION) then
            acc = real(S%counter(C_R)) / real(S%counter(C_TRIAL_R))
            if (acc - TARGET_ACCEPTANCE > TOL_ACCEPTANCE) then
                S%rotation_step = min(S%rotation_step * 1.05d0, MAX_ROTATION_ANGLE)
            else if (acc - TARGET_ACCEPTANCE < TOL_ACCEPTANCE) then
                S%rotation_step = min(S%rotation_step * 1.95d0, MIN_ROTATION_ANGLE)
            end if
        end if
    end subroutine adjust_move_step_sizes

    function pick_residue_type() result(t)
        integer :: t, n_active, k, i
        n_active = 0
        do i = 1, S%n_res
            if (S%res(i)%active == 1) n_active = n_active + 1
        end do
        t = 0
        if (n_active == 0) return
        k = int(rand_uniform() * n_active) + 1
        do i = 1, S%n_res
            if (S%res(i)%active == 1) then
                k = k - 1
                if (k == 0) then
                    t = i
                    return
                end if
            end if
        end do
    end function pick_residue_type

    !---------------------------------------------------------------------------
    ! program MANIAC from ComputeSystemEnergy on (main.f90:26-33): initial energy, MonteCarloLoop,
    ! FinalReport, with every output file.  outdir ends with '/'.  seed > 0 seeds the generator by the
    ! reference's rule; seed <= 0 leaves it as it is.  Returns the first engine status met (0 = none).
    !---------------------------------------------------------------------------
    function mchain_run(nb_block, nb_step, seed, outdir) bind(C, name="mchain_run") result(rc)
        integer(c_int), value :: nb_block, nb_step, seed
        character(kind=c_char), intent(in) :: outdir(*)
        integer(c_int) :: rc
        integer :: i, t, m, stat, step
        integer(c_int) :: cap, run_kmax, run_dmax
        integer(kind=8) :: c0, c1, crate
        real(real64) :: e6(6)
        logical :: want_gc

        S%outdir = ''
        do i = 1, len(S%outdir)
            if (outdir(i) == c_null_char) exit
            S%outdir(i:i) = outdir(i)
        end do
        S%nb_block = nb_block
        S%nb_step = nb_step
        S%counter = 0
        open(unit=S%log_unit, file=trim(S%outdir) // 'log.maniac', status='replace')
        call write_log_header(S)

        call system_clock(c0, crate)
        call ComputeSystemEnergy(S%engine, e6, stat=stat)
        call note(stat)
        call system_clock(c1)
        init_seconds = real(c1 - c0, real64) / real(crate, real64)
        file_seconds = 0.0_real64
        S%energy = e6
        if (seed > 0) call seed_rng(int(seed))

        ! the engine's one-launch window path, where it applies to this system (and the host wants it)
        chain_cap = 0
        if (fused .and. chain_windows) then
            stat = mgpu_chain_set_wide(S%engine, merge(1_c_int, 0_c_int, wide_windows))
            call note(stat)
            stat = mgpu_chain_window_capacity(S%engine, cap)
            call note(stat)
            if (stat == 0) chain_cap = int(cap)
        end if
        ! chain runs, where the host wants them, the input draws no insertion / deletion and the engine takes this system (a
        ! triclinic box: only where the caller has switched mgpu_chain_run_set_triclinic on -- the capacity says so, and the
        ! block is then driven exactly as an orthorhombic one: the engine wraps the centres, refresh_frames reads them back);
        ! elsewhere the windows above
        ! A block WITH insertions / deletions: only where the host has asked for it (mchain_set_chain_run_gcmc), the run is not
        ! --as-written and the engine takes the switch (no reservoir; a triclinic box only with triclinic runs on, which the
        ! capacity above has already said): run_block by count, for either kind of box -- the engine builds the insertion's centre
        ! (lo + box%matrix u) and wraps the translations, refresh_frames reads them back, and the fallback's windows are the
        ! ones such a box takes without runs: host-built rows through the loop's own ApplyPBC, after drop_frames.
        run_on = .false.
        run_gc = .false.
        run_fallback = 0
        want_gc = S%p_translation + S%p_rotation < one
        if (fused .and. run_k > 0 .and. .not. S%has_reservoir .and. (.not. want_gc .or. (run_gc_want .and. .not. as_written))) then
            stat = mgpu_chain_run_capacity(S%engine, run_kmax, run_dmax, run_ring)
            call note(stat)
            if (stat == 0 .and. run_kmax > 0 .and. want_gc) then
                ! (a refusal is not an error of the run: it keeps its windows)
                if (mgpu_chain_run_set_gc(S%engine, 1_c_int) /= MGPU_OK) run_kmax = 0
            end if
            if (stat == 0 .and. run_kmax > 0) then
                run_on = .true.
                run_gc = want_gc
                run_k = min(run_k, int(run_kmax))
                run_depth = min(run_depth, int(run_dmax))
                call upload_frames()
            end if
        end if
        loop_seconds = 0.0_real64

        S%current_block = 0
        call log_start_mc(S)
        call system_clock(c0, crate)
        call update_files(S, .false.)
        call system_clock(c1)
        file_seconds = file_seconds + real(c1 - c0, real64) / real(crate, real64)
        do while (S%current_block < nb_block .and. status == 0)
            S%current_block = S%current_block + 1
            step = 1
            call system_clock(c0, crate)
            if (run_on) then
                call run_block(int(nb_step), run_gc)
                step = nb_step + 1
            end if
            do while (step <= nb_step .and. status == 0)
                step = step + take_steps(nb_step - step + 1)
            end do
            call system_clock(c1)
            loop_seconds = loop_seconds + real(c1 - c0, real64) / real(crate, real64)
            call adjust_move_step_sizes()
            call system_clock(c0)
            call log_status(S)
            call update_files(S, .true.)
            call system_clock(c1)
            file_seconds = file_seconds + real(c1 - c0, real64) / real(crate, real64)
        end do
        call note(int(mgpu_synchronize(S%engine)))
        ! a Fortran do variable ends one past its limit: FinalReport prints nb_block + 1
        if (status == 0) S%current_block = nb_block + 1
        call log_final_report(S)
        close(S%log_unit)
        rc = status
    end function mchain_run

    !---------------------------------------------------------------------------
    ! Read-back for tests
    !---------------------------------------------------------------------------
    subroutine mchain_get_energy(e) bind(C, name="mchain_get_energy")
        real(c_double), intent(out) :: e(6)
        e = S%energy
    end subroutine mchain_get_energy

    subroutine mchain_get_counters(c) bind(C, name="mchain_get_counters")
        integer(c_int), intent(out) :: c(8)
        c = S%counter
    end subroutine mchain_get_counters

    subroutine mchain_get_counts(n) bind(C, name="mchain_get_counts")
        integer(c_int), intent(out) :: n(*)
        integer :: t
        do t = 1, S%n_res
            n(t) = S%res(t)%count
        end do
    end subroutine mchain_get_counts

    subroutine mchain_get_steps(steps) bind(C, name="mchain_get_steps")
        real(c_double), intent(out) :: steps(2)
        steps(1) = S%translation_step
        steps(2) = S%rotation_step
    end subroutine mchain_get_steps

    subroutine mchain_get_molecule(t, m, com, off) bind(C, name="mchain_get_molecule")
        integer(c_int), value :: t, m
        real(c_double), intent(out) :: com(3), off(3, *)
        com = S%res(t)%com(:, m)
        off(:, 1:S%res(t)%n1) = S%res(t)%off(:, :, m)
    end subroutine mchain_get_molecule

end module mc_chain
